"""Host: the surface of qt_lp_ineq_xl_batch (csrc/qt_lp_xl.h) without a GPU -- the entry is declared, exported and
bound -- and the NumPy model of the LP kernels (tests/lp_model.py, with the large kernels' pivot safeguard) on the inputs
of test_gpu_lp_xl.py: against HiGHS at the three smallest sizes, against the constructed optimum at (400, 320).  The
kernel runs the model's iteration, so inputs the model solves to 1e-9 are inputs the kernel can be held to.  N = 1023 is
left to the GPU test (the model takes half a minute there)."""
import ctypes
import os
import re

import lp_model
import lp_xl_cases as cases
import numpy as np
import pytest

from quantpy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qt_lp_ineq_xl_batch"


def test_entry_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/qtomo.h"
    assert NAME in _capi.SIGNATURES and len(_capi.SIGNATURES[NAME][1]) == m.group(1).count(",") + 1 == 13
    assert _capi.SIGNATURES[NAME] == _capi.SIGNATURES["qt_lp_ineq_large_batch"]
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    # the header comment states the sizes and the workspace in bytes
    doc = header[header.rindex("/*", 0, m.start()):m.start()]
    for word in ("1023", "QT_ERR_UNSUPPORTED", "8 388 608 + 56 M bytes", "256", "4 GB"):
        assert word in doc, word


@pytest.mark.parametrize("M,N", cases.HIGHS_SIZES)
def test_model_against_highs(M, N):
    A, C, b, ref = cases.highs_batch(M, N)
    for r in range(cases.N_RHS):
        for o in range(2):
            status, obj, iters, x = lp_model.ipm(A, b[r], C[o], pivot_rel=lp_model.LARGE_PIVOT)
            print((M, N), r, o, "model", obj, "HiGHS", ref[r, o], "difference", abs(obj - ref[r, o]), "iterations", iters)
            assert status == lp_model.OPTIMAL and iters <= 200
            assert abs(obj - ref[r, o]) <= cases.TOL * max(1.0, abs(ref[r, o]))


def test_model_reaches_the_constructed_optimum():
    A, c, b, x_opt, opt = cases.known_optimum(400, 320)
    assert np.all(A @ x_opt <= b + 1e-12)
    status, obj, iters, x = lp_model.ipm(A, b, c, pivot_rel=lp_model.LARGE_PIVOT)
    print("(400, 320) model", obj, "constructed", opt, "difference", abs(obj - opt), "iterations", iters)
    assert status == lp_model.OPTIMAL and iters <= 200
    assert abs(obj - opt) <= cases.TOL * max(1.0, abs(opt))
