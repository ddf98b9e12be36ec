"""Inputs of the tests of qt_lp_ineq_xl_batch (csrc/qt_lp_xl.h), shared by test_lp_xl_host.py (the NumPy model, no GPU)
and test_gpu_lp_xl.py (the kernel): test_gpu_lp_large.py's generator restated, HiGHS optima computed once per size, and
a program whose optimum is known by construction, for the sizes at which a HiGHS solve would take most of a minute."""
import functools

import numpy as np
from scipy.optimize import linprog

TOL = 1e-9
# (300, 256): the first N the large kernel refuses, n = 257 in phase 1; (700, 320): no multiple of 64
HIGHS_SIZES = [(300, 256), (520, 257), (700, 320)]
N_RHS = 3


def _bounded_lp(rng, M, N):
    """A x <= b with a bounded, non-empty interior: the last row is minus a positive combination of the others."""
    A = rng.standard_normal((M, N))
    A[-1] = -rng.uniform(0.1, 1.0, M - 1) @ A[:-1]
    return A, A @ rng.standard_normal(N)


def highs(c, A, b):
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs")


def random_batch(M, N, R):
    rng = np.random.default_rng(M * 100 + N)
    A, x0 = _bounded_lp(rng, M, N)
    b = x0[None, :] + rng.uniform(0.01, 1.0, (R, M))
    c = rng.standard_normal(N)
    return A, np.stack([c, -c]), b


@functools.lru_cache(maxsize=None)
def highs_batch(M, N):
    """(A, C, b, ref (N_RHS, 2)) of random_batch(M, N, N_RHS) with HiGHS's optima; every solve must succeed."""
    A, C, b = random_batch(M, N, N_RHS)
    ref = np.empty((N_RHS, 2))
    for r in range(N_RHS):
        for o in range(2):
            res = highs(C[o], A, b[r])
            assert res.status == 0
            ref[r, o] = res.fun
    for v in (A, C, b, ref):
        v.setflags(write=False)
    return A, C, b, ref


@functools.lru_cache(maxsize=None)
def known_optimum(M, N):
    """(A, c, b, x*, c . x*): N active rows with multipliers z in [0.5, 1.5], c = -A_act^T z, b = A x* + slack with
    slack 0 on the active rows and in [0.1, 1] elsewhere -- x* satisfies the optimality conditions, and the active rows
    (N random rows: independent) make it the only optimum."""
    rng = np.random.default_rng(M * 100 + N + 7)
    A = rng.standard_normal((M, N))
    x = rng.standard_normal(N)
    active = rng.choice(M, N, replace=False)
    c = -A[active].T @ rng.uniform(0.5, 1.5, N)
    slack = rng.uniform(0.1, 1.0, M)
    slack[active] = 0.0
    b = A @ x + slack
    for v in (A, c, b, x):
        v.setflags(write=False)
    return A, c, b, x, float(c @ x)
