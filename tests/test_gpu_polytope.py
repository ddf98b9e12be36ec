"""The batched LP solver (qt_lp_ineq_batch) and the two fidelity intervals built on the reference's cvxopt programs:
PolytopeStateInterval (interval.py:268-335) and MomentFidelityStateInterval (interval.py:113-160).  Expected values
come from HiGHS (scipy.optimize.linprog) and from tests/golden/polytope.npz (make_golden_polytope.py)."""
import ctypes
import json

import numpy as np
import pytest
from conftest import load_golden
from scipy.interpolate import interp1d
from scipy.optimize import linprog

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _bounded_lp(rng, M, N):
    """A x <= b with a bounded, non-empty interior: the last row is minus a positive combination of the others."""
    A = rng.standard_normal((M, N))
    A[-1] = -rng.uniform(0.1, 1.0, M - 1) @ A[:-1]
    return A, A @ rng.standard_normal(N)


def _highs(c, A, b):
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs")


@pytest.mark.parametrize("M,N", [(6, 3), (36, 15), (64, 63), (216, 63), (432, 63)])
def test_lp_batch_against_highs(M, N):
    from quantpy_amd import _capi, get_engine

    rng = np.random.default_rng(M * 100 + N)
    A, x0 = _bounded_lp(rng, M, N)
    R = 6
    b = x0[None, :] + rng.uniform(0.01, 1.0, (R, M))
    c = rng.standard_normal(N)
    C = np.stack([c, -c])
    obj, status, iters, x = get_engine(1).lp_ineq_batch(A, C, b, return_x=True)
    assert np.all(status == _capi.LP_OPTIMAL), status
    assert np.all(iters <= 200)
    for r in range(R):
        for o in range(2):
            ref = _highs(C[o], A, b[r])
            assert ref.status == 0
            assert abs(obj[r, o] - ref.fun) <= 1e-9 * max(1.0, abs(ref.fun)), (r, o, obj[r, o], ref.fun)
            assert np.all(A @ x[r, o] <= b[r] + 1e-9)
            assert abs(C[o] @ x[r, o] - obj[r, o]) <= 1e-9 * max(1.0, abs(obj[r, o]))


def test_lp_batch_status_and_errors():
    import torch

    from quantpy_amd import _capi, get_engine
    from quantpy_amd.engine import EngineError

    eng = get_engine(1)
    # infeasible: x <= -1 and -x <= -1
    A = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    obj, status, _ = eng.lp_ineq_batch(A, np.array([[1.0, 1.0]]), np.array([[-1.0, -1.0, 1.0, 1.0]]))
    assert status[0, 0] == _capi.LP_INFEASIBLE and obj[0, 0] == np.inf
    # unbounded: no lower bound on the third coordinate; the opposite objective is bounded
    A = np.vstack([np.eye(3), -np.eye(3)[:2]])
    obj, status, _ = eng.lp_ineq_batch(A, np.array([[0.3, -0.2, 1.0], [0.3, -0.2, -1.0]]), np.ones((1, 5)))
    assert status[0, 0] == _capi.LP_UNBOUNDED and obj[0, 0] == -np.inf
    assert status[0, 1] == _capi.LP_OPTIMAL and abs(obj[0, 1] - _highs([0.3, -0.2, -1.0], A, np.ones(5)).fun) < 1e-9
    # rank-deficient A: a status, no crash or hang
    rng = np.random.default_rng(5)
    A = rng.standard_normal((20, 3))
    A = np.hstack([A, A[:, :1] + A[:, 1:2]])
    _, status, _ = eng.lp_ineq_batch(A, rng.standard_normal((2, 4)), A @ rng.standard_normal(4) + 1.0)
    assert np.all(np.isin(status, [_capi.LP_NOT_CONVERGED, _capi.LP_UNBOUNDED])), status
    # N > 64, null pointers, bad sizes
    with pytest.raises(EngineError) as err:
        eng.lp_ineq_batch(rng.standard_normal((70, 65)), np.ones((1, 65)), np.ones((1, 70)))
    assert err.value.code == _capi.QT_ERR_UNSUPPORTED
    lib, h = eng.lib, eng._h
    buf = np.zeros(64)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    q = st.ctypes.data_as(ctypes.c_void_p)
    assert lib.qt_lp_ineq_batch(h, None, 4, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_batch(h, p, 4, 2, p, 1, p, 1, p, None, None, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_batch(h, p, 1, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_batch(h, p, 4, 2, p, 0, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_batch(h, p, 4, 2, p, 1, p, 0, p, None, q, None, 0) == _capi.QT_ERR_ARG
    # device pointers give the host call's results
    A, x0 = _bounded_lp(rng, 36, 15)
    b = x0[None, :] + rng.uniform(0.01, 1.0, (5, 36))
    C = rng.standard_normal((2, 15))
    obj, status, iters, x = eng.lp_ineq_batch(A, C, b, return_x=True)
    dev = torch.device("cuda", eng.device)
    tA, tC, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (A, C, b))
    tobj = torch.empty((5, 2), dtype=torch.float64, device=dev)
    tx = torch.empty((5, 2, 15), dtype=torch.float64, device=dev)
    tst = torch.empty((5, 2), dtype=torch.int32, device=dev)
    tit = torch.empty((5, 2), dtype=torch.int32, device=dev)
    eng._dev_call()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.qt_lp_ineq_batch(h, ptr(tA), 36, 15, ptr(tC), 2, ptr(tb), 5, ptr(tobj), ptr(tx), ptr(tst), ptr(tit),
                                _capi.QT_DEVICE_PTR) == 0
    eng.sync()
    assert np.array_equal(tobj.cpu().numpy(), obj) and np.array_equal(tx.cpu().numpy(), x)
    assert np.array_equal(tst.cpu().numpy(), status) and np.array_equal(tit.cpu().numpy(), iters)


def _tomograph(qp, g, name):
    counts = g[name + "/counts"]
    povm = g[name + "/povm"]
    n = int(round(np.log2(povm.shape[-1]) / 2))
    tmg = qp.StateTomograph(qp.qobj.fully_mixed(n))
    tmg.povm_matrix = povm
    tmg.results = counts
    return tmg


@pytest.mark.parametrize("name", list(load_golden("polytope")["polytope_cases"]))
def test_polytope_interval_against_reference(qp, name):
    g = load_golden("polytope")
    tmg = _tomograph(qp, g, name)
    target = qp.Qobj(g[name + "/target"])
    interval = qp.PolytopeStateInterval(tmg, n_points=int(g[name + "/n_points"]), target_state=target)
    interval.setup()
    lo_d, hi_d = g[name + "/delta_range"]
    assert np.array_equal(interval.deltas, np.linspace(lo_d, hi_d, int(g[name + "/n_points"])))
    ref_cl = g[name + "/conf_levels"]
    assert np.all(np.abs(interval.conf_levels - ref_cl) <= 1e-15 * np.abs(ref_cl))
    A, b, c, _, _ = interval.programs()
    rows, h_rows = g[name + "/lp_rows"], g[name + "/h_rows"]
    assert np.array_equal(A, g[name + "/G"]) and np.array_equal(b[h_rows], g[name + "/h"]) and np.array_equal(c, g[name + "/c"])
    # statuses of every program: HiGHS's 0 (optimal) / 2 (infeasible) against the kernel's
    assert np.array_equal(interval.lp_status == 1, g[name + "/lp_status"] == 2)
    assert np.abs(interval.dist_min[rows] - g[name + "/dist_min"]).max() <= 1e-8
    assert np.abs(interval.dist_max[rows] - g[name + "/dist_max"]).max() <= 1e-8
    # the functor at the stored deltas' confidence levels returns the reference's bounds there
    values, counts = np.unique(ref_cl, return_counts=True)
    unique = np.isin(ref_cl[rows], values[counts == 1])  # a level shared by several deltas is no single knot
    inner = rows[unique & (ref_cl[rows] > ref_cl.min()) & (ref_cl[rows] < ref_cl.max())]
    assert inner.size > 50
    (lo, hi), cl = interval(ref_cl[inner])
    assert np.array_equal(cl, ref_cl[inner])
    keep = np.isin(rows, inner)
    assert np.abs(lo - g[name + "/dist_min"][keep]).max() <= 1e-8
    assert np.abs(hi - g[name + "/dist_max"][keep]).max() <= 1e-8
    # and between the levels it is interp1d over the interval's own arrays
    levels = np.linspace(max(1e-3, ref_cl.min()), 1 - 1e-3, 57)
    (lo, hi), _ = interval(levels)
    assert np.array_equal(lo, interp1d(interval.conf_levels, interval.dist_min)(levels))
    assert np.array_equal(hi, interp1d(interval.conf_levels, interval.dist_max)(levels))


def test_polytope_interval_contains_true_fidelity(qp):
    """Wherever the true Bloch vector lies in the polytope, its fidelity (Tr(sigma rho) = 1/d + d c . x) lies between
    the bounds -- no solver needed for the expectation."""
    rng = np.random.default_rng(11)
    for trial in range(4):
        n = 1 + trial % 2
        d = 2**n
        g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        rho = g @ g.conj().T
        rho /= np.trace(rho)
        h = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        sigma = h @ h.conj().T
        sigma /= np.trace(sigma)
        true, target = qp.Qobj(rho), qp.Qobj(sigma)
        tmg = qp.StateTomograph(true)
        tmg.experiment(1000)
        interval = qp.PolytopeStateInterval(tmg, n_points=200, target_state=target)
        interval.setup()
        A, b, _, _, _ = interval.programs()
        inside = np.all(A @ true.bloch[1:] <= b + 1e-12, axis=1)
        assert inside.any()
        fid = np.real(np.trace(sigma @ rho))
        assert np.all(interval.dist_min[inside] <= fid + 1e-9)
        assert np.all(interval.dist_max[inside] >= fid - 1e-9)


def test_polytope_interval_quirks_and_limits(qp):
    np.random.seed(3)
    tmg = qp.StateTomograph(qp.Qobj(np.diag([0.7, 0.3])))
    tmg.experiment(1000)
    (lo, hi), _ = qp.PolytopeStateInterval(tmg, n_points=50, target_state=qp.qobj.fully_mixed(1))()
    assert np.all(lo == 1.0) and np.all(hi == 1.0)  # c = 0: every optimum is exactly 0.0, which the reference maps to 1
    proc = qp.ProcessTomograph(qp.channel.depolarizing(n_qubits=1))
    with pytest.raises(NotImplementedError, match="state tomography"):
        qp.PolytopeStateInterval(proc)
    with pytest.raises(NotImplementedError, match="state tomography"):
        qp.MomentFidelityStateInterval(proc)
    t4 = qp.StateTomograph(qp.qobj.fully_mixed(4))
    t4.experiment(100)
    with pytest.raises(NotImplementedError, match="n <= 3"):
        qp.PolytopeStateInterval(t4, n_points=10).setup()
    # not informationally complete: the z basis only
    tz = qp.StateTomograph(qp.qobj.fully_mixed(1))
    tz.experiment(100, np.array([[[0.5, 0, 0, 0.5], [0.5, 0, 0, -0.5]]]))
    with pytest.raises(ValueError, match="Rank"):
        qp.PolytopeStateInterval(tz, n_points=10).setup()


@pytest.mark.parametrize("name", list(load_golden("polytope")["moment_cases"]))
def test_moment_fidelity_against_reference(qp, name):
    g = load_golden("polytope")
    tmg = _tomograph(qp, g, name)
    target = qp.Qobj(g[name + "/target"]) if bool(g[name + "/with_target"]) else None
    interval = qp.MomentFidelityStateInterval(tmg, target_state=target)
    interval.setup()
    assert np.array_equal(interval.conf_levels, g[name + "/levels"])
    assert np.abs(interval.target_state.bloch - g[name + "/target"]).max() < 1e-13
    assert np.abs(interval.cl_to_dist(g[name + "/levels"]) - g[name + "/cl_to_dist"]).max() < 1e-10
    assert np.abs(interval.dist_min - g[name + "/dist_min"]).max() < 1e-10
    assert np.abs(interval.dist_max - g[name + "/dist_max"]).max() < 1e-10
    (lo, hi), _ = interval([0.5, 0.9])
    assert np.all(lo <= hi)


def test_state_interval_cli_with_target(qp, tmp_path):
    from quantpy_amd import cli

    povm = qp.generate_measurement_matrix("proj-set", 1)
    data = {"povm_matrix": np.asarray(povm).tolist(), "outcomes": [[5002, 4998], [5028, 4972], [9990, 10]],
            "conf_levels": [0.5, 0.9, 0.99], "target_state": [[1, 0], [0, 0]]}
    src = tmp_path / "state.json"
    src.write_text(json.dumps(data))
    out = tmp_path / "out.json"
    cli.state_interval(["-i", str(src), "-o", str(out)])
    res = json.load(open(out))
    tmg = qp.StateTomograph(qp.qobj.fully_mixed(1))
    tmg.povm_matrix = povm
    tmg.results = np.asarray(data["outcomes"])
    tmg.point_estimate(physical=False)
    interval = qp.MomentFidelityStateInterval(tmg, target_state=qp.Qobj(np.array(data["target_state"], dtype=complex)))
    (lo, hi), _ = interval(data["conf_levels"])
    assert np.allclose(res["fidelity_min"], np.maximum(lo, 0), rtol=0, atol=1e-14)
    assert np.allclose(res["fidelity_max"], np.minimum(hi, 1), rtol=0, atol=1e-14)
    assert max(res["fidelity_max"]) <= 1.0 and min(res["fidelity_min"]) >= 0.0
    plain = qp.MomentInterval(tmg)
    plain.setup()
    assert np.allclose(res["hs_radius"], plain.cl_to_dist(data["conf_levels"]), rtol=0, atol=1e-14)
