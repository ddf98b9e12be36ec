"""The NumPy model of the LP kernels (tests/lp_model.py) against HiGHS on the hard programs of tests/lp_cases.py: the
small kernel's list with its plain Cholesky, the large kernel's and the XL kernel's with the pivot safeguard.  No GPU.  This is what
test_gpu_lp_hard.py rests on: the algorithm alone stays within a fifth of that test's tolerance on every case, so a
kernel that misses it there differs from the algorithm and not merely in its summation order."""
import lp_cases
import lp_model
import numpy as np
import pytest

HOST_TOL = 2e-10  # a fifth of the GPU test's 1e-9


def _check(kind, name, pivot_rel):
    cs = lp_cases.case(kind, name)
    ref_status, ref, how = lp_cases.reference(kind, name)
    status, obj, iters, x = lp_model.ipm(cs.A, cs.b, cs.c, pivot_rel=pivot_rel)
    diff = abs(obj - ref) if np.isfinite(ref) and np.isfinite(obj) else np.nan
    print(name, cs.A.shape, "reference", how, ref_status, "model", status, "iterations", iters, "|obj - ref|", diff,
          "relative", diff / max(1.0, abs(ref)))
    assert ref_status == cs.status  # the reference says what the family was built to be
    return cs, ref, status, obj, iters, x


def _check_optimum(cs, ref, obj, x):
    assert abs(obj - ref) <= lp_cases.objective_bound(ref, HOST_TOL), (obj, ref)
    if cs.exact is not None:
        assert abs(obj - cs.exact) <= lp_cases.objective_bound(cs.exact, HOST_TOL), (obj, cs.exact)
    assert (cs.A @ x - cs.b).max() <= lp_cases.violation_bound(cs.A, cs.b, x, 1e-9)


@pytest.mark.parametrize("name", lp_cases.names("small"))
def test_model_without_safeguard_on_the_small_list(name):
    cs, ref, status, obj, iters, x = _check("small", name, None)
    if cs.family == "dual_degenerate" and cs.status == lp_model.OPTIMAL:
        # what Engine._lp_ineq_by_size rests on: the plain Cholesky breaks down where c is a facet's normal
        assert status == lp_model.NOT_CONVERGED and np.isnan(obj)
        return
    assert status == cs.status and iters <= 200
    if status == lp_model.OPTIMAL:
        _check_optimum(cs, ref, obj, x)


@pytest.mark.parametrize("name", lp_cases.names("large"))
def test_model_with_safeguard_on_the_large_list(name):
    cs, ref, status, obj, iters, x = _check("large", name, lp_model.LARGE_PIVOT)
    assert status == cs.status and iters <= 200
    if status == lp_model.OPTIMAL:
        _check_optimum(cs, ref, obj, x)


@pytest.mark.parametrize("name", [n for n in lp_cases.names("xl") if n != lp_cases.XL_FULL[0]])
def test_model_with_safeguard_on_the_xl_list(name):
    """The full-width half-box (XL_FULL) is left out: the model takes 11 s there; its run (OPTIMAL, 9 iterations,
    1.0e-14 off -1) is filed in profiles/lp_xl_hard_cases.txt."""
    cs, ref, status, obj, iters, x = _check("xl", name, lp_model.LARGE_PIVOT)
    assert status == cs.status and iters <= 200
    if status == lp_model.OPTIMAL:
        _check_optimum(cs, ref, obj, x)


def test_threshold_of_the_safeguard_matters_on_these_cases():
    """With the safeguard's threshold at 0 (only a non-positive pivot is replaced, a pivot of rounding noise is kept)
    the model loses dual-degenerate programs of the large list that it solves at LARGE_PIVOT: the cases can tell the two
    apart.  Which ones depends on the BLAS's rounding, so only that it happens is asserted."""
    statuses = {}
    for name in lp_cases.names("large"):
        cs = lp_cases.case("large", name)
        if cs.family == "dual_degenerate" and cs.status == lp_model.OPTIMAL and cs.N <= 129:
            with np.errstate(all="ignore"):  # the factor overflows where a noise pivot is kept
                statuses[name] = lp_model.ipm(cs.A, cs.b, cs.c, pivot_rel=0.0)[0]
    print("threshold 0:", {k: v for k, v in statuses.items() if v != lp_model.OPTIMAL})
    assert lp_model.NOT_CONVERGED in statuses.values()
    assert set(statuses.values()) <= {lp_model.OPTIMAL, lp_model.NOT_CONVERGED}


def test_status_codes_are_the_model_s():
    from quantpy_amd import _capi

    assert (_capi.LP_OPTIMAL, _capi.LP_INFEASIBLE, _capi.LP_UNBOUNDED, _capi.LP_NOT_CONVERGED) == (
        lp_model.OPTIMAL, lp_model.INFEASIBLE, lp_model.UNBOUNDED, lp_model.NOT_CONVERGED)


def test_case_lists_cover_every_family_and_size():
    for kind, sizes in (("small", lp_cases.SMALL_N), ("large", lp_cases.LARGE_N), ("xl", lp_cases.XL_N)):
        seen = {(lp_cases.case(kind, n).family, lp_cases.case(kind, n).N) for n in lp_cases.names(kind)
                if n != lp_cases.XL_FULL[0]}
        assert {v for v in seen if v[0] != "row_objective"} == {(f, N) for f in lp_cases.FAMILIES for N in sizes}
    # sizes the kernels' seams sit at: the small kernel's cap, and both sides of the large kernel's panels and tiles
    assert 64 in lp_cases.SMALL_N and {64, 65, 96, 97, 128, 129, 255} <= set(lp_cases.LARGE_N)
    assert min(lp_cases.XL_N) > 256 and min(lp_cases.XL_N) >= lp_cases.SHARED_FROM  # above the large kernel; solves shared
    full = lp_cases.case("xl", lp_cases.XL_FULL[0])
    assert full.A.shape == (2045, 1023) and full.exact == -1.0 and lp_cases.reference("xl", full.name)[1:] == (-1.0, "exact")
    for kind in ("large", "xl"):
        for name in lp_cases.names(kind):
            cs = lp_cases.case(kind, name)
            assert cs.A.shape[0] >= cs.N and cs.A.shape == (cs.b.size, cs.c.size)
    # the programs are the same in every process: fixed seeds
    a = lp_cases.case("small", "row_scaled-N15")
    lp_cases._cases.cache_clear()
    b = lp_cases.case("small", "row_scaled-N15")
    assert a.A is not b.A and np.array_equal(a.A, b.A) and np.array_equal(a.b, b.b) and np.array_equal(a.c, b.c)


@pytest.mark.parametrize("family", ["row_scaled", "col_scaled", "duplicated", "offset"])
def test_shared_reference_is_the_family_s_own(family):
    """From N = 224 on these families take the `random` case's HiGHS optimum (moved by c . x1 for offset).  At N = 129,
    where both are cheap, that equals HiGHS on the case itself well inside the bound."""
    N = 129
    cs = lp_cases.case("large", "%s-N%d" % (family, N))
    own = lp_cases.reference("large", cs.name)
    base = lp_cases.reference("large", "random-N%d" % N)
    shift = getattr(lp_cases, family)(N, lp_cases.rows_of("large", N))[3] if family == "offset" else 0.0
    assert own[2] == "highs" and own[0] == base[0] == lp_model.OPTIMAL
    print(family, "own", own[1], "shared", base[1] + shift, "difference", abs(own[1] - base[1] - shift))
    assert abs(own[1] - (base[1] + shift)) <= 1e-11 * max(1.0, abs(own[1]))
    big = lp_cases.case("large", "%s-N255" % family)
    assert big.base is not None and lp_cases.reference("large", big.name)[2] == "shared"
