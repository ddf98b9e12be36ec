"""GPU: trace distance and infidelity of a batch against a table of centres (qt_metric_dist_group_batch,
Engine.metric_dist / metric_dist_dev, geometry.trace_dst_batch / if_dst_batch; reference geometry.py:23-56).

The values are checked against a float64 restatement this file owns (eigvalsh / eigh of Hermitian arguments) and against
the reference's own numbers, the 24 pairs geo{i}_a, geo{i}_b of tests/golden/leftovers.npz (d = 2, 4, 8: full-rank,
rank-deficient, pure, identical and near-identical).  Tolerances:
* trace distance against the restatement 1e-13: d eigenvalues of a matrix of norm <= 2, a few ulp each.
* infidelity against the restatement 1e-12 where both operands have full rank (`matrix_rank(., 1e-10) == d`), 1e-6
  otherwise: up to d zero eigenvalues of S rho S, each off by a few ulp of ||M|| <= 1, contribute sqrt(1e-15) ~ 3e-8 apiece
  to the root fidelity and twice that to F -- the project's 1e-6 infidelity convention.
* against the golden values 1e-12 for full pairs, and 1e-7 (trace) / 1e-6 (infidelity) for the others, where the
  reference's sqrtm is itself off by 1.4e-8 / 2.4e-8 from the restatement.
The layout tests compare bits: a trial's value depends on its two matrices alone."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

METRICS = ("trace", "if")
TPB = {1: 64, 2: 16, 3: 4}  # trials per workgroup


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


@pytest.fixture(scope="module")
def golden():
    z = load_golden("leftovers")
    pairs = []
    for i in range(int(z["geo_n_pairs"])):
        a, b = z[f"geo{i}_a"], z[f"geo{i}_b"]
        d = a.shape[0]
        full = np.linalg.matrix_rank(a, 1e-10) == d and np.linalg.matrix_rank(b, 1e-10) == d
        pairs.append(dict(a=a, b=b, d=d, full=full, same=np.array_equal(a, b), trace=float(z[f"geo{i}_trace"]),
                          **{"if": float(z[f"geo{i}_if"])}))
    assert len(pairs) == 24 and sum(p["same"] for p in pairs) == 3
    return pairs


# ---- 1. the reference's pairs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_reference_pairs(golden, metric):
    import quantpy_amd as qp

    for k, p in enumerate(golden):
        eng = qp.get_engine(int(np.log2(p["d"])))
        got = eng.metric_dist(p["a"], p["b"], metric)
        own = REF[metric](p["a"], p["b"])
        print(f"pair {k} d={p['d']} full={p['full']} {metric}: got {got!r} restated {own!r} golden {p[metric]!r}")
        if metric == "trace":
            tol_own, tol_gold = 1e-13, (1e-12 if p["full"] else 1e-7)
        else:
            tol_own, tol_gold = (1e-12, 1e-12) if p["full"] else (1e-6, 1e-6)
        assert abs(got - own) <= tol_own, (k, got, own)
        assert abs(got - p[metric]) <= tol_gold, (k, got, p[metric])
        if p["same"]:
            assert got == 0.0 and not np.signbit(got), (k, got)
        # symmetric in its arguments, to the same tolerance (the engine takes the root of the SECOND one)
        assert abs(eng.metric_dist(p["b"], p["a"], metric) - own) <= tol_own


# ---- 2. layout -----------------------------------------------------------------------------------------------------------
def _full_rank(g, count, d):
    m = g.standard_normal((count, d, d)) + 1j * g.standard_normal((count, d, d))
    rho = m @ m.conj().transpose(0, 2, 1)
    return rho / np.trace(rho, axis1=1, axis2=2).real[:, None, None]


@pytest.fixture(scope="module")
def batches():
    """n -> (rho (BMAX, d, d), centres (3, d, d), single[metric][c] (BMAX,): trial b against centre c, one call each)."""
    import quantpy_amd as qp

    out = {}
    for n in (1, 2, 3):
        g = np.random.default_rng(40 + n)
        d, bmax = 2**n, 2 * TPB[n] + 3
        rho, cen = _full_rank(g, bmax, d), _full_rank(g, 3, d)
        eng = qp.get_engine(n)
        single = {m: np.array([[eng.metric_dist(r, c, m) for r in rho] for c in cen]) for m in METRICS}
        out[n] = (rho, cen, single)
    return out


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_single_calls_match_the_restatement(batches, n, metric):
    rho, cen, single = batches[n]
    want = np.array([[REF[metric](r, c) for r in rho] for c in cen])
    assert np.abs(single[metric] - want).max() <= (1e-13 if metric == "trace" else 1e-12)
    # distinct pairs: a wrong centre or a wrong trial shows
    assert (single[metric] > 1e-9).all() and len(np.unique(single[metric])) == single[metric].size


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_batched_call_equals_single_calls(batches, n, metric):
    import quantpy_amd as qp

    rho, cen, single = batches[n]
    eng = qp.get_engine(n)
    for b in (1, TPB[n] - 1, TPB[n] + 1, 2 * TPB[n] + 3):
        got = eng.metric_dist(rho[:b], cen[1], metric)
        assert got.shape == (b,) and np.array_equal(_bits(got), _bits(single[metric][1, :b])), (b, got)
        # a table of G = 3 centres entered at g0 = 2: trial t against centre (2 + t) % 3
        got = eng.metric_dist(rho[:b], cen, metric, g0=2)
        want = single[metric][(2 + np.arange(b)) % 3, np.arange(b)]
        assert np.array_equal(_bits(got), _bits(want)), (b, got, want)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_device_pointers_equal_host_pointers(batches, n, metric):
    import torch

    import quantpy_amd as qp

    rho, cen, single = batches[n]
    eng = qp.get_engine(n)
    b = rho.shape[0]
    r_d, c_d = torch.from_numpy(rho).cuda(), torch.from_numpy(cen).cuda()
    dist = torch.full((b + 3,), -7.0, dtype=torch.float64, device="cuda")
    eng.metric_dist_dev(r_d, c_d, dist[:b], metric, g0=2)
    eng.sync()
    dist = dist.cpu().numpy()
    assert (dist[b:] == -7.0).all()  # nothing behind row B
    assert np.array_equal(_bits(dist[:b]), _bits(eng.metric_dist(rho, cen, metric, g0=2)))
    eng.metric_dist_dev(r_d, c_d[0], dist_one := torch.empty(b, dtype=torch.float64, device="cuda"), metric)
    eng.sync()
    assert np.array_equal(_bits(dist_one.cpu().numpy()), _bits(single[metric][0]))


# ---- 3. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_nan_stays_in_its_trial(batches, n, metric):
    import quantpy_amd as qp

    rho, cen, single = batches[n]
    eng = qp.get_engine(n)
    for where in ((0, 1), (1, 1)):  # an off-diagonal and a diagonal element
        bad = rho.copy()
        bad[1][where] = np.nan
        got = eng.metric_dist(bad, cen[0], metric)
        assert np.isnan(got[1])
        keep = np.arange(len(rho)) != 1
        assert np.array_equal(_bits(got[keep]), _bits(single[metric][0][keep]))
    # a NaN in one centre of a table: the trials measured against it, and no others
    bad = cen.copy()
    bad[1, 0, -1] = np.nan
    got = eng.metric_dist(rho, bad, metric)
    hit = np.arange(len(rho)) % 3 == 1
    assert np.isnan(got[hit]).all()
    assert np.array_equal(_bits(got[~hit]), _bits(single[metric][np.arange(len(rho)) % 3, np.arange(len(rho))][~hit]))


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def test_return_codes():
    import quantpy_amd as qp
    from quantpy_amd import _capi

    eng = qp.get_engine(2)
    rho = np.ascontiguousarray(_full_rank(np.random.default_rng(0), 3, 4))
    dist = np.full(3, -7.0)
    call = eng.lib.qt_metric_dist_group_batch
    tr = _capi.QT_METRIC_TRACE
    assert call(eng._h, 2, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # unknown metric
    assert call(eng._h, -1, _ptr(rho), 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, _ptr(rho), 3, _ptr(rho), 0, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # G < 1
    assert call(eng._h, tr, _ptr(rho), 3, _ptr(rho), 3, 3, _ptr(dist), 0) == _capi.QT_ERR_ARG  # g0 outside [0, G)
    assert call(eng._h, tr, _ptr(rho), 3, _ptr(rho), 3, -1, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, None, 3, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG  # null arrays with B > 0
    assert call(eng._h, tr, _ptr(rho), 3, None, 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, _ptr(rho), 3, _ptr(rho), 1, 0, None, 0) == _capi.QT_ERR_ARG
    assert call(eng._h, tr, _ptr(rho), -1, _ptr(rho), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_ARG
    for metric in (tr, _capi.QT_METRIC_INFIDELITY):
        assert call(eng._h, metric, None, 0, None, 1, 0, None, 0) == 0  # B == 0: nothing to do
    assert (dist == -7.0).all()
    for n in (4, 5):
        big = qp.get_engine(n)
        m = np.zeros((1, 2**n, 2**n), dtype=np.complex128)
        assert call(big._h, tr, _ptr(m), 1, _ptr(m), 1, 0, _ptr(dist), 0) == _capi.QT_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="metric"):
        eng.metric_dist(rho, rho[0], "hs")


@pytest.mark.parametrize("metric", METRICS)
def test_handle_without_a_povm(batches, metric):
    from quantpy_amd.engine import Engine

    rho, cen, single = batches[2]
    eng = Engine(2, stream="own")  # a handle of its own: qt_set_povm has never been called on it
    try:
        assert np.array_equal(_bits(eng.metric_dist(rho, cen[0], metric)), _bits(single[metric][0]))
    finally:
        eng.close()


def test_batch_functions_on_qobj_lists(batches):
    import quantpy_amd as qp

    rho, cen, single = batches[2]
    objs = [qp.Qobj(r) for r in rho[:5]]
    for fn, metric, host, tol in ((qp.trace_dst_batch, "trace", qp.trace_dst, 1e-7), (qp.if_dst_batch, "if", qp.if_dst, 1e-6)):
        got = fn(objs, qp.Qobj(cen[0]))
        # (Qobj rebuilds its matrix from the Bloch vector: the engine sees those matrices, not rho's bits)
        want = np.array([REF[metric](o.matrix, qp.Qobj(cen[0]).matrix) for o in objs])
        assert got.shape == (5,) and np.abs(got - want).max() <= (1e-13 if metric == "trace" else 1e-12)
        assert np.abs(got - np.array([host(o, qp.Qobj(cen[0])) for o in objs])).max() <= tol
        assert np.array_equal(_bits(fn(rho[:5], cen[0])), _bits(single[metric][0][:5]))  # arrays pass as they are
    # d > 8: the host functions in a loop
    big = _full_rank(np.random.default_rng(3), 3, 16)
    assert np.array_equal(qp.trace_dst_batch(big[:2], big[2]), [qp.trace_dst(b, big[2]) for b in big[:2]])
    assert np.array_equal(qp.if_dst_batch(big[:2], big[2]), [qp.if_dst(b, big[2]) for b in big[:2]])
