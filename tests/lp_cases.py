"""Hard linear programs for the three batched LP kernels (csrc/qt_lp.h, csrc/qt_lp_large.h, csrc/qt_lp_xl.h), shared by the host test of
the NumPy model (test_lp_cases_host.py) and the GPU test (test_gpu_lp_hard.py):

    minimise c . x  subject to  A x <= b,  x free.

Every family is `family(N, M) -> (A, b, c)` (or a dict of variants), deterministic: the generator of a (family, N)
is seeded by the family's name and N, and the families that transform `random` ("random with ...") start from the
`random` program of the same size.  What each one is hard for:

    random             Gaussian A, fat interior, Gaussian c: the control (the generator of test_gpu_polytope.py)
    primal_degenerate  the box |x_i| <= 1 and max(2, N // 2) rows e . x <= sum(e), e > 0, all active at the optimum
                       x = 1 of c < 0 (N + max(2, N // 2) active rows at a vertex of R^N); optimum -sum|c| exactly
    dual_degenerate    c parallel to a row: `random` with c = -A[k] (k = 0, 5: a whole facet is optimal), and the rotated
                       half-box [I; -I[1:]] Q with c = -Q^T e_0 (optimum -1 exactly, attained on an unbounded facet);
                       variant `halfbox_unbounded` is the opposite objective
    slab               [P; -P] x <= [f + d u; -f + d u'], the shape of the polytope programs, of width d = 1e-3, 1e-6
    row_scaled         `random` with row i of A and b_i times 10^U(-3, 3): same feasible set, same optimum
    col_scaled         `random` with column j of A and c_j times 10^U(-2, 2): x_j scales, the optimum does not
    duplicated         `random` with every row twice (H is the same, the multipliers are not unique)
    offset             `random` with b + A x1, x1 = 1e4 * gaussian: the optimum moves by c . x1, far from phase 1's x = 0
    simplex            `random` with M = N + 1 rows, the fewest that bound a polytope
    infeasible         a slab (d = 1e-3) with one row's upper bound below its lower bound
    row_objective      small list only: the four dual_degenerate programs at N = 1 and 2 that are not degenerate there
                       (_ROW_OBJECTIVE); every solver finds their optimum

Sizes: the small kernel's list is N in SMALL_N with M = 3 N + 1, the large kernel's N in LARGE_N with M = 2 N + 3, where
the family leaves M free; the XL kernel's list ('xl') is N in XL_N with the large list's M, every size of it shared as
below, and one full-width program, XL_FULL: the half-box at N = 1023 (M = 2045, optimum -1 exactly), which drives the
pivot replacement at n = 1024 (profiles/lp_xl_hard_cases.txt has the model's run of it, which the host test leaves
out).  References are HiGHS's, computed once per case and process (`reference`).  At N >= 224 a
HiGHS solve takes about a second, so there the families that transform `random` share its one solve (their optimum is
the same number, or moves by c . x1), dual_degenerate keeps one of its two k and slab one of its two widths per size,
and the families whose answer is known by construction (primal_degenerate, the half-box, infeasible) are not solved at
all; `reference` says which in its third value.
"""
import functools
import zlib
from collections import namedtuple

import lp_model
import numpy as np
from scipy.optimize import linprog

SMALL_N = (1, 2, 15, 63, 64)
LARGE_N = (15, 64, 65, 96, 97, 128, 129, 224, 255)
XL_N = (257, 385)
XL_FULL = ("dual_degenerate-halfbox-N1023", 1023)
SHARED_FROM = 224  # sizes from here on share HiGHS solves (module docstring)

# name: the case's id; status: the expected lp_model / qt_lp_status; exact: the optimum known by construction or None;
# base: (name of the case whose HiGHS optimum this one shares, the shift to add to it) or None
Case = namedtuple("Case", "name family N A b c status exact base")


# A case that missed the host test's bound on its first seed draws again.  simplex at N = 255: HiGHS, not the model, is
# 3.8e-9 off the optimum found by enumerating the 256 vertices (the model 4.0e-12).
_RESEED = {("simplex", 255): 1}


def _rng(family, N):
    return np.random.default_rng([zlib.crc32(family.encode()), N, _RESEED.get((family, N), 0)])


def rows_of(kind, N):
    return 3 * N + 1 if kind == "small" else 2 * N + 3  # 'large' and 'xl'


def bounded_lp(rng, M, N):
    """test_gpu_polytope.py's generator: the last row is minus a positive combination of the others."""
    A = rng.standard_normal((M, N))
    A[-1] = -rng.uniform(0.1, 1.0, M - 1) @ A[:-1]
    return A, A @ rng.standard_normal(N)


def random(N, M):
    rng = _rng("random", N)
    A, ax0 = bounded_lp(rng, M, N)
    return A, ax0 + rng.uniform(0.01, 1.0, M), rng.standard_normal(N)


def primal_degenerate(N, M=None):
    rng = _rng("primal_degenerate", N)
    E = np.abs(rng.standard_normal((max(2, N // 2), N)))
    A = np.vstack([np.eye(N), -np.eye(N), E])
    b = np.concatenate([np.ones(2 * N), E.sum(axis=1)])
    return A, b, -rng.uniform(0.5, 1.5, N)


def _halfbox(N):
    Q = np.linalg.qr(_rng("dual_degenerate", N).standard_normal((N, N)))[0]
    return np.vstack([np.eye(N), -np.eye(N)[1:]]) @ Q, Q


def dual_degenerate_halfbox(N):
    """The rotated half-box alone (the 'halfbox' variant of dual_degenerate, without the `random` program beside it)."""
    half, Q = _halfbox(N)
    return half, np.ones(2 * N - 1), -Q[0]


def dual_degenerate(N, M):
    A, b, _ = random(N, M)
    out = {"k%d" % k: (A, b, -A[k % M]) for k in (0, 5)}
    half, Q = _halfbox(N)
    out["halfbox"] = (half, np.ones(2 * N - 1), -Q[0])
    out["halfbox_unbounded"] = (half, np.ones(2 * N - 1), Q[0].copy())
    return out


def _slab(rng, N, d):
    P = rng.standard_normal((2 * N + 1, N))
    f = P @ rng.standard_normal(N)
    upper = f + d * rng.uniform(0.5, 1.0, 2 * N + 1)
    lower = f - d * rng.uniform(0.5, 1.0, 2 * N + 1)
    return P, upper, lower, rng.standard_normal(N)


def slab(N, M=None):
    out = {}
    for tag, d in (("1e-3", 1e-3), ("1e-6", 1e-6)):
        P, upper, lower, c = _slab(_rng("slab" + tag, N), N, d)
        out[tag] = (np.vstack([P, -P]), np.concatenate([upper, -lower]), c)
    return out


def row_scaled(N, M):
    A, b, c = random(N, M)
    scale = 10.0 ** _rng("row_scaled", N).uniform(-3.0, 3.0, M)
    return A * scale[:, None], b * scale, c


def col_scaled(N, M):
    A, b, c = random(N, M)
    scale = 10.0 ** _rng("col_scaled", N).uniform(-2.0, 2.0, N)
    return A * scale[None, :], b, c * scale


def duplicated(N, M):
    A, b, c = random(N, M)
    return np.repeat(A, 2, axis=0), np.repeat(b, 2), c


def offset(N, M):
    A, b, c = random(N, M)
    x1 = 1e4 * _rng("offset", N).standard_normal(N)
    return A, b + A @ x1, c, float(c @ x1)


def simplex(N, M=None):
    rng = _rng("simplex", N)
    A, ax0 = bounded_lp(rng, N + 1, N)
    return A, ax0 + rng.uniform(0.01, 1.0, N + 1), rng.standard_normal(N)


def infeasible(N, M=None):
    rng = _rng("infeasible", N)
    d = 1e-3
    P, upper, lower, c = _slab(rng, N, d)
    k = int(rng.integers(2 * N + 1))
    upper[k] = lower[k] - d
    return np.vstack([P, -P]), np.concatenate([upper, -lower]), c


FAMILIES = ("random", "primal_degenerate", "dual_degenerate", "slab", "row_scaled", "col_scaled", "duplicated", "offset",
            "simplex", "infeasible")
# dual_degenerate's programs that are not degenerate on the small list: a 1 x 1 normal matrix never breaks down, and
# at N = 2 row 5 of the `random` program is redundant, so its normal is no facet's.  The model solves them, and they
# are kept as ordinary OPTIMAL cases of a family of their own.
_ROW_OBJECTIVE = {(1, "k0"), (1, "k5"), (1, "halfbox"), (2, "k5")}
_SHARES_RANDOM = ("row_scaled", "col_scaled", "duplicated", "offset")


@functools.lru_cache(maxsize=None)
def _cases(kind):
    out = {}
    for N in {"small": SMALL_N, "large": LARGE_N, "xl": XL_N}[kind]:
        M = rows_of(kind, N)
        shared = N >= SHARED_FROM
        for family in FAMILIES:
            made = globals()[family](N, M)
            variants = made if isinstance(made, dict) else {"": made}
            if shared and family == "dual_degenerate":
                del variants["k5" if N in (224, 257) else "k0"]
            if shared and family == "slab":
                del variants["1e-6" if N in (224, 257) else "1e-3"]
            for tag, prog in variants.items():
                name = "%s%s-N%d" % (family, "-" + tag if tag else "", N)
                A, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in prog[:3])
                status, exact, base = lp_model.OPTIMAL, None, None
                if family == "primal_degenerate":
                    exact = -np.abs(c).sum()
                elif tag == "halfbox":
                    exact = -1.0
                elif tag == "halfbox_unbounded":
                    status = lp_model.UNBOUNDED
                elif family == "infeasible":
                    status = lp_model.INFEASIBLE
                if shared and family in _SHARES_RANDOM:
                    base = ("random-N%d" % N, prog[3] if family == "offset" else 0.0)
                if kind == "small" and (N, tag) in _ROW_OBJECTIVE:
                    name, family_of = "row_objective-%s-N%d" % (tag, N), "row_objective"
                else:
                    family_of = family
                out[name] = Case(name, family_of, N, A, b, c, status, exact, base)
    if kind == "xl":
        name, N = XL_FULL
        A, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in dual_degenerate_halfbox(N))
        out[name] = Case(name, "dual_degenerate", N, A, b, c, lp_model.OPTIMAL, -1.0, None)
    return out


def names(kind):
    """Case ids of the 'small', the 'large' or the 'xl' list, in a fixed order."""
    return list(_cases(kind))


def case(kind, name):
    return _cases(kind)[name]


def highs(c, A, b):
    """HiGHS with its feasibility tolerances at 1e-10, the tightest it takes.  At its default of 1e-7 it leaves a slab
    of width 1e-6 by up to a tenth of the width, and its optimum is then off by 3e-8 (slab-1e-6 at N = 15; 4e-14 with
    these)."""
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs",
                   options={"primal_feasibility_tolerance": 1e-10, "dual_feasibility_tolerance": 1e-10})


_HIGHS_STATUS = {0: lp_model.OPTIMAL, 2: lp_model.INFEASIBLE, 3: lp_model.UNBOUNDED}


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """-> (status, optimum, how): HiGHS's answer for the case ('highs'), the `random` case's HiGHS answer moved by the
    family's exact shift ('shared'), or the answer known by construction ('exact'), as the module docstring lays out.
    The optimum is +inf / -inf for an infeasible / unbounded program, as in the kernels."""
    cs = case(kind, name)
    if cs.N >= SHARED_FROM and (cs.exact is not None or cs.status != lp_model.OPTIMAL):
        fun = {lp_model.INFEASIBLE: np.inf, lp_model.UNBOUNDED: -np.inf}.get(cs.status, cs.exact)
        return cs.status, fun, "exact"
    if cs.base is not None:
        status, fun, _ = reference(kind, cs.base[0])
        return status, fun + cs.base[1], "shared"
    res = highs(cs.c, cs.A, cs.b)
    status = _HIGHS_STATUS.get(res.status, -1)
    fun = {lp_model.OPTIMAL: res.fun, lp_model.INFEASIBLE: np.inf, lp_model.UNBOUNDED: -np.inf}.get(status, np.nan)
    return status, fun, "highs"


def objective_bound(ref, tol):
    return tol * max(1.0, abs(ref))


def violation_bound(A, b, x, tol):
    """The scale of the primal-residual test the iteration stops on (lp_phase, lp_model.phase): max(1, max|b|,
    max|A| * ||x||_1)."""
    return tol * max(1.0, np.abs(b).max(), np.abs(A).max() * np.abs(x).sum())
