"""The NumPy model of the LP kernels (tests/lp_model.py) against HiGHS, on the programs the large kernel is built for:
the polytope programs of tests/golden/polytope_fidelity.npz (a one- and a two-qubit process, a four-qubit state; their
expected optima in the fixture are HiGHS's) and the random programs of test_gpu_lp_large.py.  No GPU: this is the
evidence for the safeguard of csrc/qt_lp_large.h, which the kernel then follows."""
import lp_model
import numpy as np
import polytope_fidelity_cases as cases
import pytest
from scipy.optimize import linprog

TOL = 1e-9  # the project's bound for an LP objective against HiGHS (tests/test_gpu_polytope.py)


def _highs(c, A, b):
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs")


def _rows(g, name):
    return [int(r) for r in g[name + "/h_rows"]][:4]


@pytest.mark.parametrize("name", cases.all_cases())
def test_fixture_programs_rebuilt_on_host(name):
    """The package's host code poses the reference's programs: G at the stored rows, c, h and the deltas bit for bit."""
    g = cases.golden()
    A, b, c, deltas, freq = cases.case_programs(g, name)
    assert A.shape == tuple(g[name + "/G_shape"]) and b.shape == (int(g[name + "/n_points"]), A.shape[0])
    assert np.array_equal(A[g[name + "/G_rows"]], g[name + "/G_sample"])
    assert abs(A.sum() - g[name + "/G_sum"]) <= 1e-12 * np.abs(A).sum()
    assert abs((A * A).sum() - g[name + "/G_sumsq"]) <= 1e-12 * g[name + "/G_sumsq"]
    assert np.array_equal(c, g[name + "/c"])
    assert np.array_equal(b[g[name + "/h_rows"]], g[name + "/h"])
    assert np.array_equal(deltas[[0, -1]], g[name + "/delta_range"])
    assert np.linalg.matrix_rank(A) == A.shape[1]


@pytest.mark.parametrize("name", cases.all_cases())
def test_model_with_pivot_replacement_matches_highs(name):
    g = cases.golden()
    A, b, c, _, _ = cases.case_programs(g, name)
    ref = g[name + "/lp_obj"]
    for r in _rows(g, name):
        for o, sign in enumerate((1.0, -1.0)):
            status, obj, iters, x = lp_model.ipm(A, b[r], sign * c, pivot_rel=lp_model.LARGE_PIVOT)
            print(name, r, o, "status", status, "iterations", iters, "model", obj, "HiGHS", ref[r, o])
            assert status == lp_model.OPTIMAL and iters <= 200
            assert abs(obj - ref[r, o]) <= TOL * max(1.0, abs(ref[r, o]))
            assert np.all(A @ x <= b[r] + 1e-9)


def test_plain_cholesky_breaks_down_on_these_programs():
    """Why the large kernel has a safeguard: the small kernel's iteration, unchanged, ends most polytope programs of the
    two large sizes in a non-positive pivot (NOT_CONVERGED) although HiGHS finds their optimum."""
    g = cases.golden()
    statuses = []
    for name in ("proc2_sic_projset_1e3", "state4_ghz_projset_1e3"):
        A, b, c, _, _ = cases.case_programs(g, name)
        assert np.all(g[name + "/lp_status"] == 0)
        for r in _rows(g, name):
            statuses += [lp_model.ipm(A, b[r], sign * c)[0] for sign in (1.0, -1.0)]
    print("plain Cholesky:", statuses)
    assert lp_model.NOT_CONVERGED in statuses


def test_cholesky_replacing_is_plain_cholesky_without_small_pivots():
    rng = np.random.default_rng(3)
    B = rng.standard_normal((40, 12))
    H = B.T @ B
    L, replaced = lp_model.cholesky_replacing(H, lp_model.LARGE_PIVOT)
    assert replaced == 0 and np.abs(L - np.linalg.cholesky(H)).max() <= 1e-13 * np.abs(L).max()
    H[:, 5] = H[:, 4]
    H[5, :] = H[4, :]  # singular: one pivot vanishes and is replaced by its diagonal entry
    L, replaced = lp_model.cholesky_replacing(H, lp_model.LARGE_PIVOT)
    assert replaced == 1 and np.all(np.isfinite(L)) and L[5, 5] == np.sqrt(H[5, 5])
    with pytest.raises(np.linalg.LinAlgError):
        lp_model.cholesky_replacing(-np.eye(3), lp_model.LARGE_PIVOT)


def bounded_lp(rng, M, N):
    """test_gpu_polytope.py's generator: the last row is minus a positive combination of the others."""
    A = rng.standard_normal((M, N))
    A[-1] = -rng.uniform(0.1, 1.0, M - 1) @ A[:-1]
    return A, A @ rng.standard_normal(N)


@pytest.mark.parametrize("M,N", [(70, 65), (300, 128), (576, 240), (1296, 255)])
def test_model_on_the_random_programs_of_the_gpu_test(M, N):
    """Programs that never break down: the safeguard changes nothing, and the model meets the bound against HiGHS."""
    rng = np.random.default_rng(M * 100 + N)
    A, x0 = bounded_lp(rng, M, N)
    b = x0[None, :] + rng.uniform(0.01, 1.0, (3, M))
    c = rng.standard_normal(N)
    for r in range(3):
        for sign in (1.0, -1.0):
            plain = lp_model.ipm(A, b[r], sign * c)
            status, obj, iters, _ = lp_model.ipm(A, b[r], sign * c, pivot_rel=lp_model.LARGE_PIVOT)
            ref = _highs(sign * c, A, b[r])
            print((M, N), r, sign, "iterations", iters, "model", obj, "HiGHS", ref.fun)
            assert ref.status == 0 and status == lp_model.OPTIMAL and plain[0] == lp_model.OPTIMAL
            assert iters == plain[2] and abs(obj - plain[1]) <= 1e-12 * max(1.0, abs(obj))
            assert abs(obj - ref.fun) <= TOL * max(1.0, abs(ref.fun))


@pytest.mark.parametrize("name", ["proc2_sic_projset_1e3", "state4_ghz_projset_1e3"])
@pytest.mark.parametrize("lowered", [0.05, 0.02])
def test_model_status_on_narrowed_polytopes(name, lowered):
    """The polytope with its right-hand side lowered: infeasible or not, the model says what HiGHS says."""
    g = cases.golden()
    A, b, c, _, _ = cases.case_programs(g, name)
    rhs = b[0] - lowered
    ref = _highs(c, A, rhs)
    status, obj, iters, _ = lp_model.ipm(A, rhs, c, pivot_rel=lp_model.LARGE_PIVOT)
    print(name, lowered, "HiGHS status", ref.status, "model", status, iters)
    assert ref.status in (0, 2)
    assert status == (lp_model.OPTIMAL if ref.status == 0 else lp_model.INFEASIBLE)
    if ref.status == 0:
        assert abs(obj - ref.fun) <= TOL * max(1.0, abs(ref.fun))
