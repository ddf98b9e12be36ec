"""GPU: trace distance and infidelity of 64 x 64 matrices -- the Choi matrix of a three-qubit channel -- on any handle
(qt_metric_dist_mat, Engine.metric_dist / metric_dist_dev; reference geometry.py:23-56): one workgroup of 1024 threads per
trial, four elements per thread (csrc/qt_metric_dim64.h).  Below 64 the entry runs the code of qt_metric_dist_dim.

The fixtures and the float64 restatement (eigvalsh / eigh of Hermitian arguments) are those of
tests/test_gpu_metric_dist_dim.py at d = 64, with one more kind, "choi": the real parts of two completely positive,
trace-preserving three-qubit Choi matrices of trace 8 (a unitary channel near the identity mixed with the depolarizing
channel, built on the host).  Tolerances, that file's:
* trace distance against the restatement 1e-13 max(1, Tr);
* infidelity against the restatement 1e-12 where both operands have full rank, 1e-6 otherwise (zero eigenvalues of
  S rho S off by a few ulp contribute sqrt(1e-15) apiece to the root fidelity; a matrix with negative eigenvalues counts
  as rank-deficient where it is the second argument, whose root clips them);
* against the host functions 1e-7 (trace) / 1e-6 (infidelity), the infidelity of the matrix with negative eigenvalues
  exempt (scipy's sqrtm of it is another function).
Identical arguments: the trace distance is +0.0; the infidelity of identical full-rank 64 x 64 states is only required
within 1e-12 of 0 (float64 linear algebra itself lands anywhere in +-3e-13 there); of two Choi matrices of trace 8 it is
exactly 0.0 (1 - 64 < 1e-15).  The layout tests compare bits: a trial's value depends on its two matrices alone."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

METRICS = ("trace", "if")
D = 64
KINDS = ("full", "near", "same", "half", "clipped", "pure_full", "pure_pure", "indefinite", "choi")


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


def _choi(g, p):
    """Re of the Choi matrix (trace 8) of: with probability 1 - p a three-qubit unitary near the identity, else the fully
    depolarizing channel.  The real part of a CPTP Choi matrix is one (the mean of the channel and its conjugate)."""
    h = g.standard_normal((8, 8)) + 1j * g.standard_normal((8, 8))
    lam, u = np.linalg.eigh(h + h.conj().T)
    vec = ((u * np.exp(0.05j * lam)) @ u.conj().T).reshape(-1)
    return ((1 - p) * np.outer(vec, vec.conj()) + p / 8 * np.eye(64)).real + 0j


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
    g = np.random.default_rng(1064)
    out["choi"] = (_choi(g, 0.1), _choi(g, 0.15))
    assert tuple(out) == KINDS and (np.linalg.eigvalsh(indef) < -1e-3).sum() >= 2
    for c in out["choi"]:  # CPTP, trace 8: positive, and the partial trace over the output is the identity
        assert np.linalg.eigvalsh(c).min() > 0 and np.abs(np.einsum("ikjk->ij", c.reshape(8, 8, 8, 8)) - np.eye(8)).max() < 1e-12
    return out


def _full(d, a, b):
    """Both operands have full rank -- the second one, whose root the engine takes, after the clip of its negative
    eigenvalues that the root applies (for a positive semi-definite b: matrix_rank(b, 1e-10) == d as it stands)."""
    lam, u = np.linalg.eigh(b)
    clipped = (u * np.maximum(lam, 0)) @ u.conj().T
    return np.linalg.matrix_rank(a, 1e-10) == d and np.linalg.matrix_rank(clipped, 1e-10) == d


@pytest.fixture(scope="module")
def eng():
    """An n = 3 handle on which qt_set_povm is never called by this file."""
    from quantpy_amd.engine import Engine

    e = Engine(3, stream="own")
    yield e
    e.close()


# ---- 1. values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_values_of_every_kind(eng, metric):
    import quantpy_amd as qp

    host = {"trace": qp.trace_dst, "if": qp.if_dst}[metric]
    tol_host = {"trace": 1e-7, "if": 1e-6}[metric]
    for kind, (a, b) in pairs_of(D).items():
        got, swapped = eng.metric_dist(a, b, metric), eng.metric_dist(b, a, metric)
        own, own_swapped = REF[metric](a, b), REF[metric](b, a)
        if metric == "trace":
            tol = tol_swapped = 1e-13 * max(1.0, np.trace(a).real, np.trace(b).real)
        else:
            tol, tol_swapped = (1e-12 if _full(D, *p) else 1e-6 for p in ((a, b), (b, a)))
        by_host = float(host(a, b))
        print(f"{kind} {metric}: got {got!r} swapped {swapped!r} restated {own!r} / {own_swapped!r} host {by_host!r}"
              f" err {abs(got - own):.2e} / {abs(swapped - own_swapped):.2e} tol {tol:.0e} / {tol_swapped:.0e}")
        assert isinstance(got, float) and abs(got - own) <= tol, (kind, got, own)
        # the engine takes the root of the SECOND argument: swapped, the same tolerance
        assert abs(swapped - own_swapped) <= tol_swapped, (kind, swapped, own_swapped)
        if kind != "indefinite":  # of positive semi-definite arguments both are symmetric
            assert abs(swapped - own) <= tol, (kind, swapped, own)
        if not (kind == "indefinite" and metric == "if"):  # (see the module's docstring)
            assert abs(got - by_host) <= tol_host, (kind, got, by_host)
        if kind == "same" and metric == "trace":
            assert got == 0.0 and not np.signbit(got), got
        elif kind == "same":
            assert abs(got) <= 1e-12 and not np.signbit(got), got
        elif kind == "choi" and metric == "if":  # 1 - (~8)^2 < 1e-15
            assert got == 0.0 and swapped == 0.0 and not np.signbit(got) and not np.signbit(swapped), (got, swapped)
        else:
            assert own > 1e-9 and own_swapped > 1e-9, kind  # (the fixture: nowhere near the 1e-15 rule or the clip)


# ---- 2. layout -----------------------------------------------------------------------------------------------------------
BMAX = 5


@pytest.fixture(scope="module")
def batch(eng):
    """(rho (BMAX, 64, 64), centres (3, 64, 64), single[metric][c] (BMAX,): trial b against centre c, one call each)."""
    g = np.random.default_rng(40 + D)
    rho, cen = _wishart(g, D, count=BMAX), _wishart(g, D, count=3)
    single = {m: np.array([[eng.metric_dist(r, c, m) for r in rho] for c in cen]) for m in METRICS}
    return rho, cen, single


@pytest.mark.parametrize("metric", METRICS)
def test_single_calls_match_the_restatement(batch, metric):
    rho, cen, single = batch
    want = np.array([[REF[metric](r, c) for r in rho] for c in cen])
    err = np.abs(single[metric] - want).max()
    print(f"{metric}: max |single - restated| {err:.2e}")
    assert err <= (1e-13 if metric == "trace" else 1e-12)
    # distinct pairs: a wrong centre or a wrong trial shows
    assert (single[metric] > 1e-9).all() and len(np.unique(single[metric])) == single[metric].size


@pytest.mark.parametrize("metric", METRICS)
def test_batched_call_equals_single_calls(eng, batch, metric):
    rho, cen, single = batch
    for b in (1, 2, 5):
        got = eng.metric_dist(rho[:b], cen[1], metric)
        assert got.shape == (b,) and np.array_equal(_bits(got), _bits(single[metric][1, :b])), (b, got)
        # a table of G = 3 centres entered at g0 = 2: trial t against centre (2 + t) % 3
        got = eng.metric_dist(rho[:b], cen, metric, g0=2)
        want = single[metric][(2 + np.arange(b)) % 3, np.arange(b)]
        assert np.array_equal(_bits(got), _bits(want)), (b, got, want)


@pytest.mark.parametrize("metric", METRICS)
def test_device_pointers_equal_host_pointers(eng, batch, metric):
    import torch

    rho, cen, single = batch
    b = rho.shape[0]
    r_d, c_d = torch.from_numpy(rho).cuda(), torch.from_numpy(cen).cuda()
    buf = torch.full((b + 6,), -7.0, dtype=torch.float64, device="cuda")
    eng.metric_dist_dev(r_d, c_d, buf[3:3 + b], metric, g0=2)
    eng.sync()
    out = buf.cpu().numpy()
    assert (out[:3] == -7.0).all() and (out[3 + b:] == -7.0).all()  # nothing in front of row 0 or behind row B
    assert np.array_equal(_bits(out[3:3 + b]), _bits(single[metric][(2 + np.arange(b)) % 3, np.arange(b)]))
    eng.metric_dist_dev(r_d, c_d[0], dist_one := torch.empty(b, dtype=torch.float64, device="cuda"), metric)
    eng.sync()
    assert np.array_equal(_bits(dist_one.cpu().numpy()), _bits(single[metric][0]))


def test_infidelity_table_twice_gives_the_same_bits(eng, batch):
    """The roots of the G = 3 centres go into the handle's workspace, grown for the first call and reused by the second;
    a one-centre call in between leaves a smaller table in front of it."""
    rho, cen, single = batch
    want = single["if"][np.arange(BMAX) % 3, np.arange(BMAX)]
    first = eng.metric_dist(rho, cen, "if")
    assert np.array_equal(_bits(first), _bits(want))
    assert np.array_equal(_bits(eng.metric_dist(rho, cen, "if")), _bits(first))
    assert np.array_equal(_bits(eng.metric_dist(rho, cen[2], "if")), _bits(single["if"][2]))
    assert np.array_equal(_bits(eng.metric_dist(rho, cen, "if")), _bits(first))


# ---- 3. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_nan_stays_in_its_trial(eng, batch, metric):
    rho, cen, single = batch
    for where, what in (((0, 1), np.nan), ((1, 1), np.nan), ((63, 17), np.inf)):  # off-diagonal, diagonal, another thread's
        bad = rho.copy()
        bad[1][where] = what
        got = eng.metric_dist(bad, cen[0], metric)
        assert np.isnan(got[1])
        keep = np.arange(len(rho)) != 1
        assert np.array_equal(_bits(got[keep]), _bits(single[metric][0][keep]))
    # a NaN, then an infinity, in one centre of a table: the trials measured against it, and no others
    for what in (np.nan, -np.inf):
        bad = cen.copy()
        bad[1, 0, -1] = what
        got = eng.metric_dist(rho, bad, metric)
        hit = np.arange(len(rho)) % 3 == 1
        assert hit.sum() == 2 and np.isnan(got[hit]).all()
        assert np.array_equal(_bits(got[~hit]), _bits(single[metric][np.arange(len(rho)) % 3, np.arange(len(rho))][~hit]))


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def test_return_codes(eng):
    from quantpy_amd import _capi

    rho = np.ascontiguousarray(_wishart(np.random.default_rng(0), D, count=3))
    dist = np.full(3, -7.0)
    call = eng.lib.qt_metric_dist_mat
    tr = _capi.QT_METRIC_TRACE
    assert call(eng._h, 2, D, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # unknown metric
    assert call(eng._h, -1, D, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    for dim in (3, 128, 0, -64, 1):
        assert call(eng._h, tr, dim, _ptr(rho), 1, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_UNSUPPORTED, dim
        assert "2, 4, 8, 16, 32, 64" in eng.lib.qt_last_error().decode()  # the refusal names the supported set
    assert call(eng._h, tr, D, _ptr(rho), 3, _ptr(rho), 0, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # G < 1
    assert call(eng._h, tr, D, _ptr(rho), 3, _ptr(rho), 3, 3, _ptr(dist), 0) == _capi.QT_ERR_ARG  # g0 outside [0, G)
    assert call(eng._h, tr, D, _ptr(rho), 3, _ptr(rho), 3, -1, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, D, None, 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # null arrays with B > 0
    assert call(eng._h, tr, D, _ptr(rho), 3, None, 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, D, _ptr(rho), 3, _ptr(rho), 1, 0, None, 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, D, _ptr(rho), -1, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    for metric in (tr, _capi.QT_METRIC_INFIDELITY):
        for dim in (4, 32, 64):
            assert call(eng._h, metric, dim, None, 0, None, 1, 0, None, 0) == 0  # B == 0: nothing to do
    assert (dist == -7.0).all()
    with pytest.raises(ValueError, match="metric"):
        eng.metric_dist(rho, rho[0], "hs")


@pytest.mark.parametrize("metric", METRICS)
def test_any_handle(batch, metric):
    """A one-qubit handle of its own, on which qt_set_povm has never been called, computes d = 64."""
    from quantpy_amd.engine import Engine

    rho, cen, single = batch
    one = Engine(1, stream="own")
    try:
        assert np.array_equal(_bits(one.metric_dist(rho, cen[0], metric)), _bits(single[metric][0]))
    finally:
        one.close()


# ---- 4. the smaller dims through the new entry: the code of qt_metric_dist_dim ---------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [8, 16, 32])
def test_smaller_dims_equal_the_sibling_entry(eng, d, metric):
    from quantpy_amd import _capi

    g = np.random.default_rng(70 + d)
    rho, cen = np.ascontiguousarray(_wishart(g, d, count=3)), np.ascontiguousarray(_wishart(g, d, count=2))
    code = {"trace": _capi.QT_METRIC_TRACE, "if": _capi.QT_METRIC_INFIDELITY}[metric]
    out = {}
    for name in ("qt_metric_dist_dim", "qt_metric_dist_mat"):
        out[name] = np.full(3, -7.0)
        assert getattr(eng.lib, name)(eng._h, code, d, _ptr(rho), 3, _ptr(cen), 2, 1, _ptr(out[name]), _capi.QT_HOST_PTR) == 0
    assert np.array_equal(_bits(out["qt_metric_dist_mat"]), _bits(out["qt_metric_dist_dim"]))
    assert (out["qt_metric_dist_mat"] > 1e-9).all()
    assert np.array_equal(_bits(eng.metric_dist(rho, cen, metric, g0=1)), _bits(out["qt_metric_dist_dim"]))
