"""qt_lp_ineq_large_batch (csrc/qt_lp_large.h): the batched LP solver for 65 ... 255 variables, with
test_gpu_polytope.py's generator, tolerances and error cases.  Expected values come from HiGHS."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import linprog

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _bounded_lp(rng, M, N):
    """A x <= b with a bounded, non-empty interior: the last row is minus a positive combination of the others."""
    A = rng.standard_normal((M, N))
    A[-1] = -rng.uniform(0.1, 1.0, M - 1) @ A[:-1]
    return A, A @ rng.standard_normal(N)


def _highs(c, A, b):
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs")


def _random_batch(M, N, R):
    rng = np.random.default_rng(M * 100 + N)
    A, x0 = _bounded_lp(rng, M, N)
    b = x0[None, :] + rng.uniform(0.01, 1.0, (R, M))
    c = rng.standard_normal(N)
    return A, np.stack([c, -c]), b


@pytest.mark.parametrize("M,N", [(70, 65), (300, 128), (576, 240), (1296, 255)])
def test_lp_large_against_highs(M, N):
    """The inputs the NumPy model was checked on (test_lp_model_host.py): all OPTIMAL, objectives within 1e-9 of HiGHS."""
    from quantpy_amd import _capi, get_engine

    A, C, b = _random_batch(M, N, 3)
    obj, status, iters, x = get_engine(1).lp_ineq_large_batch(A, C, b, return_x=True)
    print((M, N), "status", status.ravel().tolist(), "iterations", iters.ravel().tolist())
    assert np.all(status == _capi.LP_OPTIMAL), status
    assert np.all(iters <= 200)
    for r in range(3):
        for o in range(2):
            ref = _highs(C[o], A, b[r])
            print((M, N), r, o, "kernel", obj[r, o], "HiGHS", ref.fun, "difference", abs(obj[r, o] - ref.fun))
            assert ref.status == 0
            assert abs(obj[r, o] - ref.fun) <= TOL * max(1.0, abs(ref.fun)), (r, o, obj[r, o], ref.fun)
            assert np.all(A @ x[r, o] <= b[r] + 1e-9)
            assert abs(C[o] @ x[r, o] - obj[r, o]) <= TOL * max(1.0, abs(obj[r, o]))


@pytest.mark.parametrize("M,N", [(36, 15), (216, 63)])
def test_both_kernels_agree_up_to_64_variables(M, N):
    from quantpy_amd import _capi, get_engine

    eng = get_engine(1)
    A, C, b = _random_batch(M, N, 6)
    small = eng.lp_ineq_batch(A, C, b, return_x=True)
    large = eng.lp_ineq_large_batch(A, C, b, return_x=True)
    assert np.all(small[1] == _capi.LP_OPTIMAL) and np.all(large[1] == _capi.LP_OPTIMAL)
    assert np.all(np.abs(small[0] - large[0]) <= TOL * np.maximum(1.0, np.abs(small[0])))
    assert np.all(large[2] <= 200)
    # the private dispatch keeps the small kernel here, bit for bit
    picked, resolved = eng._lp_ineq_by_size(A, C, b, return_x=True)
    assert all(np.array_equal(u, v) for u, v in zip(picked, small)) and not resolved.any()


def test_dispatch_takes_the_large_kernel_above_64_variables():
    from quantpy_amd import get_engine

    eng = get_engine(1)
    A, C, b = _random_batch(70, 65, 2)
    picked, resolved = eng._lp_ineq_by_size(A, C, b)
    assert all(np.array_equal(u, v) for u, v in zip(picked, eng.lp_ineq_large_batch(A, C, b))) and resolved.all()


def test_lp_large_status_and_errors():
    import torch

    from quantpy_amd import _capi, get_engine
    from quantpy_amd.engine import EngineError

    eng = get_engine(1)
    # infeasible: x <= -1 and -x <= -1
    A = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
    obj, status, _ = eng.lp_ineq_large_batch(A, np.array([[1.0, 1.0]]), np.array([[-1.0, -1.0, 1.0, 1.0]]))
    assert status[0, 0] == _capi.LP_INFEASIBLE and obj[0, 0] == np.inf
    # unbounded: no lower bound on the third coordinate; the opposite objective is bounded
    A = np.vstack([np.eye(3), -np.eye(3)[:2]])
    obj, status, _ = eng.lp_ineq_large_batch(A, np.array([[0.3, -0.2, 1.0], [0.3, -0.2, -1.0]]), np.ones((1, 5)))
    assert status[0, 0] == _capi.LP_UNBOUNDED and obj[0, 0] == -np.inf
    assert status[0, 1] == _capi.LP_OPTIMAL and abs(obj[0, 1] - _highs([0.3, -0.2, -1.0], A, np.ones(5)).fun) < 1e-9
    # the same two at a size only this kernel takes: 80 variables in a box, the first bounded from one side only
    N = 80
    box = np.vstack([np.eye(N), -np.eye(N)])
    rhs = np.ones((1, 2 * N))
    rhs_bad = rhs.copy()
    rhs_bad[0, :N] = -2.0  # x <= -2 and -x <= 1
    c = np.linspace(-1.0, 1.0, N)
    obj, status, _ = eng.lp_ineq_large_batch(box, c[None], np.vstack([rhs, rhs_bad]))
    assert status[0, 0] == _capi.LP_OPTIMAL and abs(obj[0, 0] + np.abs(c).sum()) <= TOL * np.abs(c).sum()
    assert status[1, 0] == _capi.LP_INFEASIBLE and obj[1, 0] == np.inf
    half = np.vstack([np.eye(N), -np.eye(N)[1:]])  # nothing bounds x_0 from below
    obj, status, _ = eng.lp_ineq_large_batch(half, np.stack([np.eye(N)[0], -np.eye(N)[0]]), np.ones((1, 2 * N - 1)))
    assert status[0, 0] == _capi.LP_UNBOUNDED and obj[0, 0] == -np.inf
    assert status[0, 1] == _capi.LP_OPTIMAL and abs(obj[0, 1] + 1.0) <= TOL
    # rank-deficient A: a status, no crash or hang -- small, and with a repeated column among 100
    rng = np.random.default_rng(5)
    A = rng.standard_normal((20, 3))
    A = np.hstack([A, A[:, :1] + A[:, 1:2]])
    _, status, _ = eng.lp_ineq_large_batch(A, rng.standard_normal((2, 4)), A @ rng.standard_normal(4) + 1.0)
    assert np.all(np.isin(status, [_capi.LP_NOT_CONVERGED, _capi.LP_UNBOUNDED])), status
    A = rng.standard_normal((300, 99))
    A = np.hstack([A, A[:, 7:8]])
    obj, status, _ = eng.lp_ineq_large_batch(A, rng.standard_normal((2, 100)), A @ rng.standard_normal(100) + 1.0)
    assert np.all(status == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(obj)), status
    # N > 255, null pointers, bad sizes
    with pytest.raises(EngineError) as err:
        eng.lp_ineq_large_batch(rng.standard_normal((260, 256)), np.ones((1, 256)), np.ones((1, 260)))
    assert err.value.code == _capi.QT_ERR_UNSUPPORTED
    lib, h = eng.lib, eng._h
    buf = np.zeros(64)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    q = st.ctypes.data_as(ctypes.c_void_p)
    assert lib.qt_lp_ineq_large_batch(h, None, 4, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_large_batch(h, p, 4, 2, p, 1, p, 1, p, None, None, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_large_batch(h, p, 1, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_large_batch(h, p, 4, 2, p, 0, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_large_batch(h, p, 4, 2, p, 1, p, 0, p, None, q, None, 0) == _capi.QT_ERR_ARG
    # device pointers give the host call's results
    A, C, b = _random_batch(150, 100, 5)
    obj, status, iters, x = eng.lp_ineq_large_batch(A, C, b, return_x=True)
    dev = torch.device("cuda", eng.device)
    tA, tC, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (A, C, b))
    tobj = torch.empty((5, 2), dtype=torch.float64, device=dev)
    tx = torch.empty((5, 2, 100), dtype=torch.float64, device=dev)
    tst = torch.empty((5, 2), dtype=torch.int32, device=dev)
    tit = torch.empty((5, 2), dtype=torch.int32, device=dev)
    eng._dev_call()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.qt_lp_ineq_large_batch(h, ptr(tA), 150, 100, ptr(tC), 2, ptr(tb), 5, ptr(tobj), ptr(tx), ptr(tst), ptr(tit),
                                      _capi.QT_DEVICE_PTR) == 0
    eng.sync()
    assert np.array_equal(tobj.cpu().numpy(), obj) and np.array_equal(tx.cpu().numpy(), x)
    assert np.array_equal(tst.cpu().numpy(), status) and np.array_equal(tit.cpu().numpy(), iters)
