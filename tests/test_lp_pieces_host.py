"""Host: the surface of qt_lp_pieces without a GPU -- declared, exported, bound -- and every assertion of
test_gpu_lp_pieces.py (tests/lp_pieces_cases.py) with a NumPy float64 model in the kernel's place: A.T @ (w * A),
lp_model.cholesky_replacing and np.linalg.solve.  That the model passes shows that the bounds hold for a correct
implementation on every case, and that no case which counts replaced pivots has a pivot near a threshold."""
import ctypes
import os
import re

import lp_pieces_cases as pc
import numpy as np
import pytest

from quantpy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qt_lp_pieces"


def test_entry_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/qtomo.h"
    assert NAME in _capi.SIGNATURES and len(_capi.SIGNATURES[NAME][1]) == m.group(1).count(",") + 1 == 17
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    doc = header[header.rindex("/*", 0, m.start()):m.start()]
    for word in ("0xFF", "diagnosis", "production path", "QT_ERR_UNSUPPORTED", "upper triangles", "1e-11", "1e-12"):
        assert word in doc, word


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2e-19


def test_the_lists_hold_the_seams():
    xl = {(s.M, s.N, s.p1) for s in pc.XL_SHAPES + pc.XL_FULL_SHAPES}
    assert {s[1] for s in xl} == {1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 385, 1023}
    assert {(1100, 1023, 1), (7776, 1023, 1)} <= xl
    for N in {s[1] for s in xl} - {1023}:
        assert {(N, 0), (N, 1)} <= {(s[1], s[2]) for s in xl} and (N, N, 0) in xl
    ms = {s[0] for s in xl}
    assert any(m < 16 for m in ms) and {0, 1, 15} <= {m % 16 for m in ms} and any(m % 4 for m in ms)
    assert {s.N for s in pc.LARGE_SHAPES} == {15, 64, 65, 96, 97, 128, 129, 255}
    assert all({(N, N), (2 * N + 3, N)} <= {(s.M, s.N) for s in pc.LARGE_SHAPES} for N in (15, 255))
    assert {s.N for s in pc.SMALL_SHAPES} == {1, 2, 15, 63, 64}
    guarded = {(k, s.N) for k, s, _, _ in pc.safeguard_cases()}
    assert guarded == {(pc.LARGE, 129), (pc.XL, 129), (pc.XL, 300)}
    a, b = pc.inputs(pc.Shape(70, 33, 1, 0, "random")), pc.inputs(pc.Shape(70, 33, 0, 0, "random"))
    assert all(np.array_equal(u[:v.size] if u.ndim == 1 else u, v) for u, v in zip(a, b))


def _shapes():
    seen, out = set(), []
    for _, s in pc.reference_cases():
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


@pytest.mark.parametrize("s", _shapes(), ids=pc.shape_id)
def test_model_meets_every_bound(s):
    out = pc.model(s)
    print("smallest pivot ratio of the reference:", pc.check_pivot_gap(s, pc.expected_replaced(s)))
    pc.check_all(s, out, pc.LARGE, "model")
    again = pc.model(s)
    assert all(np.array_equal(np.asarray(out[k]).view(np.uint64), np.asarray(again[k]).view(np.uint64))
               for k in ("normal", "factor", "u", "ax", "solved"))


@pytest.mark.parametrize("s", pc.agreement_shapes(), ids=pc.shape_id)
def test_agreement_bound_holds_between_two_summation_orders(s):
    """The float64 model against itself with the rows of A in reverse order: two correct implementations that sum
    differently agree within check_agreement's bounds."""
    A, w, vm, vn = pc.inputs(s)
    a = pc.model(s)
    Af = pc.bordered(A, s.p1)[::-1]
    H = Af.T @ (w[::-1, None] * Af)
    L = pc.pivot_trace(H, pc.PIVOT[0][pc.LARGE])[0]
    b = {"normal": H, "factor": L, "u": pc.colsum_sign(s) * (Af.T @ vm[::-1]), "ax": (A[:, ::-1] @ vn[:s.N][::-1]),
         "solved": np.linalg.solve(L.T, np.linalg.solve(L, vn)), "ok": 1}
    pc.check_agreement(s, a, b)


@pytest.mark.parametrize("kernel,s,ok,replaced", [pytest.param(*c, id="%s-%s" % (pc.KERNEL_NAME[c[0]], pc.shape_id(c[1])))
                                                  for c in pc.safeguard_cases()])
def test_model_on_the_safeguard_cases(kernel, s, ok, replaced):
    out = pc.model(s)
    pc.check_poison_and_shape(s, out)
    assert out["ok"] == ok
    if s.kind != "nan_w":
        pc.check_products(s, out, "model")
    if replaced is not None:
        print("smallest other pivot ratio of the reference:", pc.check_pivot_gap(s, replaced))
        pc.check_factor(s, out, pc.PIVOT[s.mode][kernel], replaced)
        pc.check_solved(s, out, against_reference=False)
