"""qt_lp_ineq_xl_batch (csrc/qt_lp_xl.h): the batched LP solver for up to 1023 variables, with test_gpu_lp_large.py's
generator, tolerance and error cases at sizes only this kernel takes.  Expected values come from HiGHS up to 320
variables and from a program with a constructed optimum at 1023 (tests/lp_xl_cases.py; test_lp_xl_host.py runs the
NumPy model on the same inputs)."""
import ctypes

import lp_xl_cases as cases
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = cases.TOL


@pytest.mark.parametrize("M,N", cases.HIGHS_SIZES)
def test_lp_xl_against_highs(M, N):
    from quantpy_amd import _capi, get_engine

    A, C, b, ref = cases.highs_batch(M, N)
    obj, status, iters, x = get_engine(1).lp_ineq_xl_batch(A, C, b, return_x=True)
    print((M, N), "status", status.ravel().tolist(), "iterations", iters.ravel().tolist())
    print((M, N), "largest difference from HiGHS", np.abs(obj - ref).max())
    assert np.all(status == _capi.LP_OPTIMAL), status
    assert np.all(iters <= 200)
    for r in range(cases.N_RHS):
        for o in range(2):
            assert abs(obj[r, o] - ref[r, o]) <= TOL * max(1.0, abs(ref[r, o])), (r, o, obj[r, o], ref[r, o])
            assert np.all(A @ x[r, o] <= b[r] + 1e-9)
            assert abs(C[o] @ x[r, o] - obj[r, o]) <= TOL * max(1.0, abs(obj[r, o]))


@pytest.mark.parametrize("M,N", [(400, 320), (1100, 1023)])
def test_lp_xl_reaches_a_constructed_optimum(M, N):
    """(1100, 1023) is the full width: n = 1024 in phase 1."""
    from quantpy_amd import _capi, get_engine

    A, c, b, x_opt, opt = cases.known_optimum(M, N)
    obj, status, iters, x = get_engine(1).lp_ineq_xl_batch(A, c[None], b[None], return_x=True)
    print((M, N), "status", status[0, 0], "iterations", iters[0, 0], "kernel", obj[0, 0], "constructed", opt, "difference",
          abs(obj[0, 0] - opt))
    assert status[0, 0] == _capi.LP_OPTIMAL and iters[0, 0] <= 200
    assert abs(obj[0, 0] - opt) <= TOL * max(1.0, abs(opt))
    assert np.all(A @ x[0, 0] <= b + 1e-9)
    assert abs(c @ x[0, 0] - obj[0, 0]) <= TOL * max(1.0, abs(obj[0, 0]))


@pytest.mark.parametrize("M,N", [(300, 128), (1296, 255)])
def test_xl_and_large_kernels_agree_up_to_255_variables(M, N):
    """n below the XL kernel's block sizes (128 columns of H per block, 256 threads per vector sweep)."""
    from quantpy_amd import _capi, get_engine

    eng = get_engine(1)
    A, C, b = cases.random_batch(M, N, 3)
    large = eng.lp_ineq_large_batch(A, C, b, return_x=True)
    xl = eng.lp_ineq_xl_batch(A, C, b, return_x=True)
    print((M, N), "largest difference", np.abs(large[0] - xl[0]).max(), "iterations", xl[2].ravel().tolist())
    assert np.all(large[1] == _capi.LP_OPTIMAL) and np.all(xl[1] == _capi.LP_OPTIMAL)
    assert np.all(np.abs(large[0] - xl[0]) <= TOL * np.maximum(1.0, np.abs(large[0])))
    assert np.all(xl[2] <= 200)


def test_dispatch_takes_the_xl_kernel_above_255_variables():
    from quantpy_amd import get_engine

    eng = get_engine(1)
    A, C, b = cases.random_batch(300, 256, 2)
    picked, resolved = eng._lp_ineq_by_size(A, C, b, return_x=True)
    assert all(np.array_equal(u, v) for u, v in zip(picked, eng.lp_ineq_xl_batch(A, C, b, return_x=True)))
    assert resolved.all()
    A, C, b = cases.random_batch(70, 65, 2)
    picked, resolved = eng._lp_ineq_by_size(A, C, b)
    assert all(np.array_equal(u, v) for u, v in zip(picked, eng.lp_ineq_large_batch(A, C, b))) and resolved.all()


def test_lp_xl_status_and_errors():
    import torch

    from quantpy_amd import _capi, get_engine
    from quantpy_amd.engine import EngineError

    eng = get_engine(1)
    # 300 variables in a box; the box made infeasible; the first variable bounded from one side only
    N = 300
    box = np.vstack([np.eye(N), -np.eye(N)])
    rhs = np.ones((1, 2 * N))
    rhs_bad = rhs.copy()
    rhs_bad[0, :N] = -2.0  # x <= -2 and -x <= 1
    c = np.linspace(-1.0, 1.0, N)
    obj, status, _ = eng.lp_ineq_xl_batch(box, c[None], np.vstack([rhs, rhs_bad]))
    assert status[0, 0] == _capi.LP_OPTIMAL and abs(obj[0, 0] + np.abs(c).sum()) <= TOL * np.abs(c).sum()
    assert status[1, 0] == _capi.LP_INFEASIBLE and obj[1, 0] == np.inf
    half = np.vstack([np.eye(N), -np.eye(N)[1:]])  # nothing bounds x_0 from below
    obj, status, _ = eng.lp_ineq_xl_batch(half, np.stack([np.eye(N)[0], -np.eye(N)[0]]), np.ones((1, 2 * N - 1)))
    assert status[0, 0] == _capi.LP_UNBOUNDED and obj[0, 0] == -np.inf
    assert status[0, 1] == _capi.LP_OPTIMAL and abs(obj[0, 1] + 1.0) <= TOL
    # rank-deficient A: a status, no crash or hang -- a repeated column among 300
    rng = np.random.default_rng(5)
    A = rng.standard_normal((700, 299))
    A = np.hstack([A, A[:, 7:8]])
    obj, status, _ = eng.lp_ineq_xl_batch(A, rng.standard_normal((2, 300)), A @ rng.standard_normal(300) + 1.0)
    assert np.all(status == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(obj)), status
    # N > 1023, null pointers, bad sizes
    with pytest.raises(EngineError) as err:
        eng.lp_ineq_xl_batch(np.zeros((1030, 1024)), np.ones((1, 1024)), np.ones((1, 1030)))
    assert err.value.code == _capi.QT_ERR_UNSUPPORTED
    lib, h = eng.lib, eng._h
    buf = np.zeros(64)
    st = np.zeros(4, dtype=np.int32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    q = st.ctypes.data_as(ctypes.c_void_p)
    assert lib.qt_lp_ineq_xl_batch(h, None, 4, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_xl_batch(h, p, 4, 2, p, 1, p, 1, p, None, None, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_xl_batch(h, p, 1, 2, p, 1, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_xl_batch(h, p, 4, 2, p, 0, p, 1, p, None, q, None, 0) == _capi.QT_ERR_ARG
    assert lib.qt_lp_ineq_xl_batch(h, p, 4, 2, p, 1, p, 0, p, None, q, None, 0) == _capi.QT_ERR_ARG
    # device pointers give the host call's results
    M, N = 300, 256
    A, C, b = cases.random_batch(M, N, 2)
    obj, status, iters, x = eng.lp_ineq_xl_batch(A, C, b, return_x=True)
    dev = torch.device("cuda", eng.device)
    tA, tC, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (A, C, b))
    tobj = torch.empty((2, 2), dtype=torch.float64, device=dev)
    tx = torch.empty((2, 2, N), dtype=torch.float64, device=dev)
    tst = torch.empty((2, 2), dtype=torch.int32, device=dev)
    tit = torch.empty((2, 2), dtype=torch.int32, device=dev)
    eng._dev_call()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.qt_lp_ineq_xl_batch(h, ptr(tA), M, N, ptr(tC), 2, ptr(tb), 2, ptr(tobj), ptr(tx), ptr(tst), ptr(tit),
                                   _capi.QT_DEVICE_PTR) == 0
    eng.sync()
    assert np.array_equal(tobj.cpu().numpy(), obj) and np.array_equal(tx.cpu().numpy(), x)
    assert np.array_equal(tst.cpu().numpy(), status) and np.array_equal(tit.cpu().numpy(), iters)
