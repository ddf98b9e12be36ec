"""The primitives of the three LP kernels one by one (qt_lp_pieces, csrc/qt_lp_pieces.hip): the normal matrix, its
Cholesky factor with the pivot safeguard, A^T v, A y and the triangular solves of LpSmall (csrc/qt_lp.h), LpLarge
(csrc/qt_lp_large.h) and LpXl (csrc/qt_lp_xl.h) against longdouble references, at a-priori rounding bounds
(tests/lp_pieces_cases.py; test_lp_pieces_host.py shows that a correct float64 implementation meets them on every case).
Through a whole solve these are invisible: the interior-point iteration corrects a wrong Newton direction and only
takes longer.  Every test prints its largest error over its bound ("LPPIECES ...")."""
import functools

import lp_pieces_cases as pc
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OUTPUTS = ("normal", "factor", "u", "ax", "solved")


@pytest.fixture(scope="module")
def eng():
    from quantpy_amd import get_engine

    return get_engine(1)


@functools.lru_cache(maxsize=None)
def _run(kernel, s):
    from quantpy_amd import get_engine

    A, w, vm, vn = pc.inputs(s)
    return get_engine(1).lp_pieces(kernel, A, w, vm, vn, p1=bool(s.p1), mode=s.mode)


def _bits(v):
    return np.ascontiguousarray(v).view(np.uint64)


def _id(v):
    return pc.shape_id(v) if isinstance(v, pc.Shape) else None


def _kernel_id(k):
    return pc.KERNEL_NAME[k]


def _case(kernel, s, *rest):
    return pytest.param(kernel, s, *rest, id="%s-%s" % (pc.KERNEL_NAME[kernel], pc.shape_id(s)))


@pytest.mark.parametrize("kernel,s", [_case(*c) for c in pc.reference_cases()])
def test_pieces_against_the_reference(eng, kernel, s):
    pc.check_all(s, _run(kernel, s), kernel, pc.KERNEL_NAME[kernel])


@pytest.mark.parametrize("s", pc.agreement_shapes(), ids=_id)
def test_kernels_agree(eng, s):
    kernels = pc.kernels_of(s)
    assert len(kernels) >= 2
    for k in kernels[1:]:
        print("LPPIECES", pc.KERNEL_NAME[kernels[0]], "against", pc.KERNEL_NAME[k])
        pc.check_agreement(s, _run(kernels[0], s), _run(k, s))


@pytest.mark.parametrize("kernel,s,ok,replaced", [_case(*c) for c in pc.safeguard_cases()])
def test_safeguard(eng, kernel, s, ok, replaced):
    """A column repeated exactly: mode 0 replaces exactly that pivot, the rank test (mode 1) refuses; a zero column and
    a NaN weight are breakdowns in both."""
    out = _run(kernel, s)
    pc.check_poison_and_shape(s, out)
    print("LPPIECES", pc.KERNEL_NAME[kernel], pc.shape_id(s), "ok", out["ok"])
    assert out["ok"] == ok
    if s.kind != "nan_w":
        pc.check_products(s, out, pc.KERNEL_NAME[kernel])
    if replaced is not None:
        pc.check_factor(s, out, pc.PIVOT[s.mode][kernel], replaced)
        pc.check_solved(s, out, against_reference=False)


@pytest.mark.parametrize("N,p1", [(15, 0), (64, 1)])
def test_small_kernel_on_a_repeated_column(eng, N, p1):
    """The plain Cholesky meets a pivot of rounding noise of either sign: it breaks down (ok = 0), or it goes on with a
    finite factor.  Nothing non-finite is handed out as a success."""
    s = pc.Shape(3 * N + 1, N, p1, 0, "repeat")
    out = _run(pc.SMALL, s)
    pc.check_poison_and_shape(s, out)
    pc.check_products(s, out, "small")
    print("LPPIECES small", pc.shape_id(s), "ok", out["ok"])
    if out["ok"]:
        low = np.tri(N + p1, dtype=bool)
        assert np.all(np.isfinite(out["factor"][low])) and np.all(np.isfinite(out["solved"]))


@pytest.mark.parametrize("kernel,s", [_case(pc.SMALL, pc.Shape(46, 15, 1, 0, "random")),
                                      _case(pc.LARGE, pc.Shape(261, 129, 1, 0, "random")),
                                      _case(pc.XL, pc.Shape(300, 257, 1, 0, "random")),
                                      _case(pc.XL, pc.Shape(603, 300, 0, 0, "repeat"))])
def test_two_calls_give_the_same_bits(eng, kernel, s):
    """Also across a call on other inputs in between, which leaves its H in the workspace."""
    A, w, vm, vn = pc.inputs(s)
    first = eng.lp_pieces(kernel, A, w, vm, vn, p1=bool(s.p1), mode=s.mode)
    other = pc.Shape(s.M + 5, s.N - 1, 1 - s.p1, 0, "random")
    eng.lp_pieces(kernel, *pc.inputs(other), p1=bool(other.p1))
    second = eng.lp_pieces(kernel, A, w, vm, vn, p1=bool(s.p1), mode=s.mode)
    assert first["ok"] == second["ok"]
    for name in OUTPUTS:
        assert np.array_equal(_bits(first[name]), _bits(second[name])), name


@pytest.mark.parametrize("kernel", [pc.SMALL, pc.LARGE, pc.XL], ids=_kernel_id)
def test_device_pointers_give_the_host_call_s_bits(eng, kernel):
    import torch

    from quantpy_amd import _capi

    s = pc.Shape(70, 33, 1, 0, "random")
    A, w, vm, vn = pc.inputs(s)
    host = eng.lp_pieces(kernel, A, w, vm, vn, p1=True)
    n = s.N + 1
    dev = {k: torch.as_tensor(np.array(v), device="cuda") for k, v in (("A", A), ("w", w), ("vm", vm), ("vn", vn))}
    out = {"normal": torch.zeros((n, n), dtype=torch.float64, device="cuda"),
           "factor": torch.zeros((n, n), dtype=torch.float64, device="cuda"),
           "u": torch.zeros(n, dtype=torch.float64, device="cuda"), "ax": torch.zeros(s.M, dtype=torch.float64, device="cuda"),
           "solved": torch.zeros(n, dtype=torch.float64, device="cuda")}
    ok = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr()  # noqa: E731
    assert eng.lib.qt_lp_pieces(eng._h, kernel, ptr(dev["A"]), s.M, s.N, ptr(dev["w"]), ptr(dev["vm"]), ptr(dev["vn"]), 1, 0,
                                ptr(out["normal"]), ptr(out["factor"]), ptr(out["u"]), ptr(out["ax"]), ptr(out["solved"]),
                                ptr(ok), _capi.QT_DEVICE_PTR) == 0
    eng.sync()
    assert int(ok.cpu()[0]) == host["ok"] == 1
    for name in OUTPUTS:
        assert np.array_equal(_bits(out[name].cpu().numpy()), _bits(host[name])), name
    # outputs that are not wanted are not written, and the others do not depend on them
    only = eng.lib.qt_lp_pieces(eng._h, kernel, ptr(dev["A"]), s.M, s.N, ptr(dev["w"]), ptr(dev["vm"]), ptr(dev["vn"]), 1, 0,
                                None, None, ptr(out["u"]), None, None, None, _capi.QT_DEVICE_PTR)
    eng.sync()
    assert only == 0 and np.array_equal(_bits(out["u"].cpu().numpy()), _bits(host["u"]))


def test_sizes_are_refused_as_by_the_lp_entries(eng):
    from quantpy_amd import _capi

    lib, h = eng.lib, eng._h
    d = np.ones(8)
    p = d.ctypes.data
    args = lambda kernel, M, N, p1=0, mode=0: lib.qt_lp_pieces(h, kernel, p, M, N, p, p, p, p1, mode, None, None, None, None,  # noqa: E731
                                                                None, None, 0)
    assert args(0, 70, 65) == args(1, 260, 256) == args(2, 1030, 1024) == _capi.QT_ERR_UNSUPPORTED
    assert args(0, 1, 2) == args(1, 4, 0) == args(3, 4, 2) == args(-1, 4, 2) == _capi.QT_ERR_ARG
    assert args(1, 4, 2, p1=2) == args(1, 4, 2, mode=2) == args(1, 4, 2, p1=1, mode=1) == _capi.QT_ERR_ARG
    assert lib.qt_lp_pieces(h, 1, None, 4, 2, p, p, p, 0, 0, None, None, None, None, None, None, 0) == _capi.QT_ERR_ARG
