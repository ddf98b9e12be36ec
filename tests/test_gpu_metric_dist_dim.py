"""GPU: trace distance and infidelity of dim x dim matrices on any handle (qt_metric_dist_dim, Engine.metric_dist_dim /
metric_dist_dim_dev; reference geometry.py:23-56): dim 16 and 32 by one workgroup per trial, dim 2, 4, 8 by the kernels of
qt_metric_dist_group_batch.

The values are checked against a float64 restatement this file owns (eigvalsh / eigh of Hermitian arguments, that of
tests/test_gpu_metric_dist.py) and against the host functions `trace_dst` / `if_dst`, on seeded pairs of every kind at
d = 16 and 32: full rank, near-identical, identical, rank d/2, PSD-clipped, pure against full rank, pure against pure, and
a Hermitian matrix with negative eigenvalues.  The tolerances are those of tests/test_gpu_metric_dist.py:
* trace distance against the restatement 1e-13;
* infidelity against the restatement 1e-12 where both operands have full rank (`matrix_rank(., 1e-10) == d`), 1e-6
  otherwise (zero eigenvalues of S rho S off by a few ulp contribute sqrt(1e-15) apiece to the root fidelity).  The matrix
  with negative eigenvalues counts as rank-deficient where it is the SECOND argument: the root clips its negative
  eigenvalues, so S rho S has that many zero eigenvalues, the case the 1e-6 is for; as the first argument it has full rank;
* against the host functions 1e-7 (trace) / 1e-6 (infidelity).  Not for the infidelity of the matrix with negative
  eigenvalues: the host takes scipy's sqrtm of it, whose imaginary eigenvalues enter |Tr .|^2, where the engine (and the
  restatement) clip them to 0 -- a different function of such an argument, by 1e-2 here.
The layout tests compare bits: a trial's value depends on its two matrices alone."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ("trace", "if")
DIMS = (16, 32)
KINDS = ("full", "near", "same", "half", "clipped", "pure_full", "pure_pure", "indefinite")


def _trace_ref(a, b):
    v = 0.5 * np.abs(np.linalg.eigvalsh(a - b)).sum()
    return 0.0 if v < 1e-15 else v


def _if_ref(a, b):
    """1 - (sum sqrt(max(mu, 0)))^2, mu the eigenvalues of the Hermitian part of S a S, S the clipped root of b."""
    lam, u = np.linalg.eigh(b)
    s = (u * np.sqrt(np.maximum(lam, 0))) @ u.conj().T
    m = s @ a @ s
    mu = np.linalg.eigvalsh(0.5 * (m + m.conj().T))
    v = 1.0 - np.sqrt(np.maximum(mu, 0)).sum() ** 2
    return 0.0 if v < 1e-15 else v


REF = {"trace": _trace_ref, "if": _if_ref}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _wishart(g, d, rank=None, count=None):
    """G G^dagger / Tr of complex Ginibre matrices G (d x rank): full rank by default, pure for rank = 1."""
    shape = (d, rank or d) if count is None else (count, d, rank or d)
    m = g.standard_normal(shape) + 1j * g.standard_normal(shape)
    rho = m @ np.swapaxes(m.conj(), -1, -2)
    return rho / np.trace(rho, axis1=-2, axis2=-1).real[..., None, None]


def _clipped(g, d):
    """A state plus Hermitian noise, its negative eigenvalues set to 0, renormalised (what a clipped 'lin' estimate is)."""
    h = g.standard_normal((d, d)) + 1j * g.standard_normal((d, d))
    lam, u = np.linalg.eigh(_wishart(g, d, rank=2) + 0.02 * (h + h.conj().T) / d)
    lam = np.maximum(lam, 0)
    return (u * (lam / lam.sum())) @ u.conj().T


def pairs_of(d):
    """kind -> (a, b), seeded."""
    g = np.random.default_rng(1000 + d)
    a, a2 = _wishart(g, d), _wishart(g, d)
    h = g.standard_normal((d, d)) + 1j * g.standard_normal((d, d))
    # Hermitian, trace near 1, noise of spectral radius ~ 2 / d (twice a state's mean eigenvalue): a third of its eigenvalues
    # are negative, and its root "fidelity" to a state stays below 1, so the infidelity is not clipped to 0
    indef = a - (h + h.conj().T) / (2 * d**1.5)
    out = {
        "full": (a, _wishart(g, d)),
        "near": (0.999 * a + 0.001 * a2, a),
        "same": (a2, a2.copy()),
        "half": (_wishart(g, d, d // 2), _wishart(g, d, d // 2)),
        "clipped": (_clipped(g, d), _clipped(g, d)),
        "pure_full": (_wishart(g, d, 1), _wishart(g, d)),
        "pure_pure": (_wishart(g, d, 1), _wishart(g, d, 1)),
        "indefinite": (indef, _wishart(g, d)),
    }
    assert tuple(out) == KINDS and (np.linalg.eigvalsh(indef) < -1e-3).sum() >= 2
    return out


def _full(d, a, b):
    """Both operands have full rank -- the second one, whose root the engine takes, after the clip of its negative
    eigenvalues that the root applies (for a positive semi-definite b: matrix_rank(b, 1e-10) == d as it stands)."""
    lam, u = np.linalg.eigh(b)
    clipped = (u * np.maximum(lam, 0)) @ u.conj().T
    return np.linalg.matrix_rank(a, 1e-10) == d and np.linalg.matrix_rank(clipped, 1e-10) == d


@pytest.fixture(scope="module")
def eng():
    """An n = 5 handle on which qt_set_povm is never called by this file."""
    from quantpy_amd.engine import Engine

    e = Engine(5, stream="own")
    yield e
    e.close()


# ---- 1. values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_values_of_every_kind(eng, d, metric):
    import quantpy_amd as qp

    host = {"trace": qp.trace_dst, "if": qp.if_dst}[metric]
    tol_host = {"trace": 1e-7, "if": 1e-6}[metric]
    for kind, (a, b) in pairs_of(d).items():
        got, swapped = eng.metric_dist_dim(a, b, metric), eng.metric_dist_dim(b, a, metric)
        own, own_swapped = REF[metric](a, b), REF[metric](b, a)
        tol, tol_swapped = (1e-13, 1e-13) if metric == "trace" else (1e-12 if _full(d, *p) else 1e-6 for p in ((a, b), (b, a)))
        by_host = float(host(a, b))
        print(f"d={d} {kind} {metric}: got {got!r} swapped {swapped!r} restated {own!r} / {own_swapped!r} host {by_host!r}")
        assert isinstance(got, float) and abs(got - own) <= tol, (kind, got, own)
        # the engine takes the root of the SECOND argument: swapped, the same tolerance
        assert abs(swapped - own_swapped) <= tol_swapped, (kind, swapped, own_swapped)
        if kind != "indefinite":  # of positive semi-definite arguments both are symmetric
            assert abs(swapped - own) <= tol, (kind, swapped, own)
        if not (kind == "indefinite" and metric == "if"):  # (see the module's docstring)
            assert abs(got - by_host) <= tol_host, (kind, got, by_host)
        if kind == "same":
            assert got == 0.0 and not np.signbit(got), got
        else:
            assert own > 1e-9 and own_swapped > 1e-9, kind  # (the fixture: nowhere near the 1e-15 rule or the clip)


# ---- 2. small dims: the kernels of qt_metric_dist_group_batch, on a handle of another size -----------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [2, 4, 8])
def test_small_dims_equal_the_group_entry(eng, d, metric):
    import quantpy_amd as qp

    g = np.random.default_rng(50 + d)
    b = 70  # more than one workgroup at every size (64 / 16 / 4 trials per workgroup)
    rho, cen = _wishart(g, d, count=b), _wishart(g, d, count=3)
    small = qp.get_engine(int(np.log2(d)))
    assert np.array_equal(_bits(eng.metric_dist_dim(rho, cen, metric, g0=1)), _bits(small.metric_dist(rho, cen, metric, g0=1)))
    assert np.array_equal(_bits(eng.metric_dist_dim(rho, cen[2], metric)), _bits(small.metric_dist(rho, cen[2], metric)))
    one = eng.metric_dist_dim(rho[3], cen[2], metric)
    assert isinstance(one, float) and one == small.metric_dist(rho[3], cen[2], metric) and one > 1e-9


# ---- 3. layout -----------------------------------------------------------------------------------------------------------
BMAX = 5


@pytest.fixture(scope="module")
def batches(eng):
    """d -> (rho (BMAX, d, d), centres (3, d, d), single[metric][c] (BMAX,): trial b against centre c, one call each)."""
    out = {}
    for d in DIMS:
        g = np.random.default_rng(40 + d)
        rho, cen = _wishart(g, d, count=BMAX), _wishart(g, d, count=3)
        single = {m: np.array([[eng.metric_dist_dim(r, c, m) for r in rho] for c in cen]) for m in METRICS}
        out[d] = (rho, cen, single)
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_single_calls_match_the_restatement(batches, d, metric):
    rho, cen, single = batches[d]
    want = np.array([[REF[metric](r, c) for r in rho] for c in cen])
    assert np.abs(single[metric] - want).max() <= (1e-13 if metric == "trace" else 1e-12)
    # distinct pairs: a wrong centre or a wrong trial shows
    assert (single[metric] > 1e-9).all() and len(np.unique(single[metric])) == single[metric].size


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_batched_call_equals_single_calls(eng, batches, d, metric):
    rho, cen, single = batches[d]
    for b in (1, 2, 5):
        got = eng.metric_dist_dim(rho[:b], cen[1], metric)
        assert got.shape == (b,) and np.array_equal(_bits(got), _bits(single[metric][1, :b])), (b, got)
        # a table of G = 3 centres entered at g0 = 2: trial t against centre (2 + t) % 3
        got = eng.metric_dist_dim(rho[:b], cen, metric, g0=2)
        want = single[metric][(2 + np.arange(b)) % 3, np.arange(b)]
        assert np.array_equal(_bits(got), _bits(want)), (b, got, want)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_device_pointers_equal_host_pointers(eng, batches, d, metric):
    import torch

    rho, cen, single = batches[d]
    b = rho.shape[0]
    r_d, c_d = torch.from_numpy(rho).cuda(), torch.from_numpy(cen).cuda()
    dist = torch.full((b + 3,), -7.0, dtype=torch.float64, device="cuda")
    eng.metric_dist_dim_dev(r_d, c_d, dist[:b], metric, g0=2)
    eng.sync()
    dist = dist.cpu().numpy()
    assert (dist[b:] == -7.0).all()  # nothing behind row B
    assert np.array_equal(_bits(dist[:b]), _bits(single[metric][(2 + np.arange(b)) % 3, np.arange(b)]))
    eng.metric_dist_dim_dev(r_d, c_d[0], dist_one := torch.empty(b, dtype=torch.float64, device="cuda"), metric)
    eng.sync()
    assert np.array_equal(_bits(dist_one.cpu().numpy()), _bits(single[metric][0]))


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", DIMS)
def test_nan_stays_in_its_trial(eng, batches, d, metric):
    rho, cen, single = batches[d]
    for where in ((0, 1), (1, 1)):  # an off-diagonal and a diagonal element
        bad = rho.copy()
        bad[1][where] = np.nan
        got = eng.metric_dist_dim(bad, cen[0], metric)
        assert np.isnan(got[1])
        keep = np.arange(len(rho)) != 1
        assert np.array_equal(_bits(got[keep]), _bits(single[metric][0][keep]))
    # a NaN in one centre of a table: the trials measured against it, and no others
    bad = cen.copy()
    bad[1, 0, -1] = np.nan
    got = eng.metric_dist_dim(rho, bad, metric)
    hit = np.arange(len(rho)) % 3 == 1
    assert hit.sum() == 2 and np.isnan(got[hit]).all()
    assert np.array_equal(_bits(got[~hit]), _bits(single[metric][np.arange(len(rho)) % 3, np.arange(len(rho))][~hit]))


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def test_return_codes(eng):
    from quantpy_amd import _capi

    rho = np.ascontiguousarray(_wishart(np.random.default_rng(0), 16, count=3))
    dist = np.full(3, -7.0)
    call = eng.lib.qt_metric_dist_dim
    tr = _capi.QT_METRIC_TRACE
    assert call(eng._h, 2, 16, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # unknown metric
    assert call(eng._h, -1, 16, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    for dim in (3, 64, 0, -16, 1):
        assert call(eng._h, tr, dim, _ptr(rho), 1, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_UNSUPPORTED, dim
    assert "2, 4, 8, 16, 32" in eng.lib.qt_last_error().decode()  # the refusal names the supported set
    assert call(eng._h, tr, 16, _ptr(rho), 3, _ptr(rho), 0, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # G < 1
    assert call(eng._h, tr, 16, _ptr(rho), 3, _ptr(rho), 3, 3, _ptr(dist), 0) == _capi.QT_ERR_ARG  # g0 outside [0, G)
    assert call(eng._h, tr, 16, _ptr(rho), 3, _ptr(rho), 3, -1, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, 16, None, 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # null arrays with B > 0
    assert call(eng._h, tr, 16, _ptr(rho), 3, None, 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, 16, _ptr(rho), 3, _ptr(rho), 1, 0, None, 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, 16, _ptr(rho), -1, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    for metric in (tr, _capi.QT_METRIC_INFIDELITY):
        for dim in (4, 16, 32):
            assert call(eng._h, metric, dim, None, 0, None, 1, 0, None, 0) == 0  # B == 0: nothing to do
    assert (dist == -7.0).all()
    with pytest.raises(ValueError, match="metric"):
        eng.metric_dist_dim(rho, rho[0], "hs")


@pytest.mark.parametrize("metric", METRICS)
def test_any_handle(batches, metric):
    """A one-qubit handle of its own, on which qt_set_povm has never been called, computes d = 16."""
    from quantpy_amd.engine import Engine

    rho, cen, single = batches[16]
    one = Engine(1, stream="own")
    try:
        assert np.array_equal(_bits(one.metric_dist_dim(rho, cen[0], metric)), _bits(single[metric][0]))
    finally:
        one.close()
