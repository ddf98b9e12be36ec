"""The three batched LP kernels (qt_lp_ineq_batch, csrc/qt_lp.h; qt_lp_ineq_large_batch, csrc/qt_lp_large.h;
qt_lp_ineq_xl_batch, csrc/qt_lp_xl.h) on the hard programs of tests/lp_cases.py -- degenerate, thin, ill-scaled, at the
kernels' seams (the small kernel's cap of 64 variables, the large kernel's 32-column panels and 64-column tiles, the XL
kernel's 256-thread strides and 128-column blocks) -- and on launches in which a persistent workgroup
solves one program after another.  Expected optima are HiGHS's (lp_cases.reference); test_lp_cases_host.py shows that
the algorithm itself (tests/lp_model.py) stays within a fifth of TOL on every case.

Every test prints one line per program (kernel, case, status, iterations, |obj - ref|, largest A x - b); the largest
differences per family are filed in profiles/lp_hard_cases.txt."""
import lp_cases
import lp_model
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9  # the bound of the existing LP tests (test_gpu_polytope.py, test_gpu_lp_large.py)


@pytest.fixture(scope="module")
def eng():
    from quantpy_amd import get_engine

    return get_engine(1)


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint64) if v.dtype == np.float64 else v


def _same_bits(u, v):
    return all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(u, v))


def _check_case(kernel, cs, ref, obj, status, iters, x, allowed=None):
    """The assertions of one program against its reference.  allowed: further statuses that pass (with a NaN objective)."""
    from quantpy_amd import _capi

    diff = abs(obj - ref) if np.isfinite(obj) and np.isfinite(ref) else np.nan
    viol = (cs.A @ x - cs.b).max() if np.all(np.isfinite(x)) else np.nan
    print("LPHARD", kernel, cs.family, cs.name, cs.A.shape, "status", status, "iterations", iters, "|obj - ref|", diff,
          "relative", diff / max(1.0, abs(ref)), "max(A x - b)", viol)
    assert 1 <= iters <= 200
    if allowed and status in allowed:
        assert status == _capi.LP_NOT_CONVERGED and np.isnan(obj)
        return
    assert status == cs.status, (status, cs.status)
    if status == _capi.LP_INFEASIBLE:
        assert obj == np.inf
    elif status == _capi.LP_UNBOUNDED:
        assert obj == -np.inf
    else:
        bound = lp_cases.objective_bound(ref, TOL)
        assert abs(obj - ref) <= bound, (obj, ref)
        if cs.exact is not None:
            assert abs(obj - cs.exact) <= lp_cases.objective_bound(cs.exact, TOL), (obj, cs.exact)
        assert abs(cs.c @ x - obj) <= bound
        assert viol <= lp_cases.violation_bound(cs.A, cs.b, x, TOL), viol


def _solve_case(fn, cs):
    obj, status, iters, x = fn(cs.A, cs.c[None], cs.b[None], return_x=True)
    return obj[0, 0], int(status[0, 0]), int(iters[0, 0]), x[0, 0]


@pytest.mark.parametrize("name", lp_cases.names("large"))
def test_large_kernel_on_hard_programs(eng, name):
    cs = lp_cases.case("large", name)
    ref_status, ref, _ = lp_cases.reference("large", name)
    assert ref_status == cs.status
    _check_case("large", cs, ref, *_solve_case(eng.lp_ineq_large_batch, cs))


@pytest.mark.parametrize("name", lp_cases.names("xl"))
def test_xl_kernel_on_hard_programs(eng, name):
    import time

    cs = lp_cases.case("xl", name)
    ref_status, ref, _ = lp_cases.reference("xl", name)
    assert ref_status == cs.status
    t0 = time.perf_counter()
    res = _solve_case(eng.lp_ineq_xl_batch, cs)
    print("LPHARD xl", name, "seconds %.2f" % (time.perf_counter() - t0))
    _check_case("xl", cs, ref, *res)


@pytest.mark.parametrize("name", lp_cases.names("small"))
def test_small_kernel_on_hard_programs(eng, name):
    """Never a wrong OPTIMAL: where c is a facet's normal the plain Cholesky may break down (NOT_CONVERGED, NaN), and
    the model does; an OPTIMAL meets the bound like any other."""
    from quantpy_amd import _capi

    cs = lp_cases.case("small", name)
    ref_status, ref, _ = lp_cases.reference("small", name)
    assert ref_status == cs.status
    gives_up = cs.family == "dual_degenerate" and cs.status == _capi.LP_OPTIMAL
    _check_case("small", cs, ref, *_solve_case(eng.lp_ineq_batch, cs),
                allowed=(_capi.LP_NOT_CONVERGED,) if gives_up else None)


def _degenerate_up_to_64():
    return [(kind, n) for kind in ("small", "large") for n in lp_cases.names(kind)
            if lp_cases.case(kind, n).family == "dual_degenerate" and lp_cases.case(kind, n).N <= 64
            and lp_cases.case(kind, n).status == lp_model.OPTIMAL]


# The one dual-degenerate program that k_lp_ineq does not give up on, although the model does: at N = 2 the breakdown
# hangs on the last bit of a 2 x 2 factorisation, and the kernel solves the half-box to 1.0e-12 in 8 iterations.
SOLVED_BY_SMALL = {("small", "dual_degenerate-halfbox-N2")}


@pytest.mark.parametrize("kind,name", _degenerate_up_to_64())
def test_dispatch_resolves_dual_degenerate_programs(eng, kind, name):
    """Engine._lp_ineq_by_size: what the small kernel gives up on, the large kernel's safeguard solves, and `resolved`
    says so.  It gives up on every case (as the model does, test_lp_cases_host.py) but the one of SOLVED_BY_SMALL,
    whose answer test_small_kernel_on_hard_programs allows; that answer then stands and is not `resolved`."""
    from quantpy_amd import _capi

    cs = lp_cases.case(kind, name)
    _, ref, _ = lp_cases.reference(kind, name)
    gave_up = eng.lp_ineq_batch(cs.A, cs.c[None], cs.b[None])[1][0, 0] == _capi.LP_NOT_CONVERGED
    (obj, status, iters, x), resolved = eng._lp_ineq_by_size(cs.A, cs.c[None], cs.b[None], return_x=True)
    _check_case("by_size", cs, ref, obj[0, 0], int(status[0, 0]), int(iters[0, 0]), x[0, 0])
    assert bool(gave_up) == ((kind, name) not in SOLVED_BY_SMALL)
    assert resolved.tolist() == [bool(gave_up)]


def test_dispatch_resolves_only_the_rows_that_need_it(eng):
    """Five right-hand sides, two of them with a NaN: those two go to the large kernel (and stay NOT_CONVERGED there),
    the other three keep the small kernel's bits."""
    from quantpy_amd import _capi

    rng = np.random.default_rng(515)
    M, N = 46, 15
    A, ax0 = lp_cases.bounded_lp(rng, M, N)
    b = ax0[None, :] + rng.uniform(0.01, 1.0, (5, M))
    b[1, 7] = np.nan
    b[3, M - 1] = np.nan
    C = rng.standard_normal((2, N))
    own = eng.lp_ineq_batch(A, C, b, return_x=True)
    picked, resolved = eng._lp_ineq_by_size(A, C, b, return_x=True)
    assert resolved.tolist() == [False, True, False, True, False]
    keep = ~resolved
    assert _same_bits([v[keep] for v in picked], [v[keep] for v in own])
    assert np.all(picked[1][keep] == _capi.LP_OPTIMAL)
    assert np.all(picked[1][resolved] == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(picked[0][resolved]))
    assert np.all(own[1][resolved] == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(own[0][resolved]))


CYCLE = 9  # right-hand sides per cycle; coprime to every grid / O below, so a workgroup's programs differ


def _nine_rhs(rng, A, feasible, infeasible):
    """Seven distinct feasible right-hand sides, an infeasible one and one with a NaN entry -> (rhs (9, M), the index of
    the infeasible one, of the NaN one)."""
    b = np.stack([feasible(rng) for _ in range(7)] + [infeasible(rng), feasible(rng)])
    b[8, A.shape[0] // 2] = np.nan
    return b[[0, 7, 1, 2, 8, 3, 4, 5, 6]], 1, 4


def _grid(kernel, M, P):
    """lp_ineq_entry's launch: min(programs, 2 048, 256 MB / the workgroup's workspace), the workspace being
    LpSmall::ws_doubles(M) = 6 M and LpLarge::ws_doubles(M) = 256 * 256 + 7 M doubles; for the XL kernel
    min(programs, 256, 4 GB / the workspace), LpXl::ws_doubles(M) = 1024 * 1024 + 7 M doubles."""
    if kernel == "xl":
        return min(P, 256, (4 << 30) // (8 * (1024 * 1024 + 7 * M)))
    return min(P, 2048, (256 << 20) // (8 * (256 * 256 + 7 * M if kernel == "large" else 6 * M)))


def _entry(eng, kernel):
    return {"small": eng.lp_ineq_batch, "large": eng.lp_ineq_large_batch, "xl": eng.lp_ineq_xl_batch}[kernel]


def _followed(status, grid):
    """lp_run gives workgroup g the programs g, g + grid, ...: program lp >= grid runs behind lp - grid.
    -> the set of (predecessor's status, own status) over all of them."""
    flat = status.ravel()
    assert flat.size > grid
    return set(zip(flat[:-grid].tolist(), flat[grid:].tolist()))


def _check_isolation(fn, A, C, rhs, R, alone=None):
    """One launch of R right-hand sides (rhs, cycled) times C's objectives against every (b, c) alone in its own launch
    (R = 1, O = 1): obj, status, iters and x bit for bit.  -> (the launch's results, the cache of lone results)."""
    alone = {} if alone is None else alone
    O = C.shape[0]
    b = rhs[np.arange(R) % rhs.shape[0]]
    res = fn(A, C, b, return_x=True)
    for k in range(rhs.shape[0]):
        for o in range(O):
            if (k, o) not in alone:
                alone[k, o] = [v[0, 0] for v in fn(A, C[o][None], rhs[k][None], return_x=True)]
            rows = np.arange(k, R, rhs.shape[0])
            for got, want in zip(res, alone[k, o]):
                want = np.broadcast_to(want, got[rows, o].shape)
                assert np.array_equal(_bits(got[rows, o]), _bits(want)), (k, o)
    return res, alone


def _isolation(eng, kernel, M, N, R):
    from quantpy_amd import _capi

    OPT, INF, UNB, NC = _capi.LP_OPTIMAL, _capi.LP_INFEASIBLE, _capi.LP_UNBOUNDED, _capi.LP_NOT_CONVERGED
    fn = _entry(eng, kernel)
    rng = np.random.default_rng(1000 * M + N)
    # a bounded polytope: u^T A = 0 for a u > 0, so A x <= A x0 - 1 has no solution
    A, _ = lp_cases.bounded_lp(rng, M, N)
    rhs, at_inf, at_nan = _nine_rhs(rng, A, lambda g: A @ g.standard_normal(N) + g.uniform(0.01, 1.0, M),
                                    lambda g: A @ g.standard_normal(N) - 1.0)
    c = rng.standard_normal(N)
    C = np.stack([c, -c, rng.standard_normal(N)])
    grid = _grid(kernel, M, 2 * R)
    assert 2 * R > grid and (grid // 2) % CYCLE != 0 and grid % 2 == 0
    (obj, status, iters, x), alone = _check_isolation(fn, A, C[:2], rhs, R)
    followed = _followed(status, grid)
    print("LPISOLATION", kernel, (M, N), "programs", 2 * R, "workgroups", grid, "statuses",
          np.bincount(status.ravel(), minlength=4).tolist(), "iterations", iters.min(), "...", iters.max(),
          "(predecessor, own) statuses", sorted(followed))
    cycle = np.arange(R) % CYCLE
    ok = (cycle != at_inf) & (cycle != at_nan)
    assert np.all(status[ok] == OPT)
    assert np.all(status[cycle == at_inf] == INF) and np.all(obj[cycle == at_inf] == np.inf)
    assert np.all(status[cycle == at_nan] == NC) and np.all(np.isnan(obj[cycle == at_nan]))
    assert np.all(iters[cycle == at_nan] == 1)
    # a feasible program did run behind an infeasible and behind a NaN one on its workgroup, and the other way round
    assert {(INF, OPT), (NC, OPT), (OPT, INF), (OPT, NC), (OPT, OPT)} <= followed
    for k in range(CYCLE):  # the lone results are right, so every program of the launch is
        if k not in (at_inf, at_nan):
            for o in range(2):
                ref = lp_cases.highs(C[o], A, rhs[k])
                assert ref.status == 0 and abs(alone[k, o][0] - ref.fun) <= TOL * max(1.0, abs(ref.fun))
    # three objectives, one pass over the nine right-hand sides: program r * O + o keeps its place
    _check_isolation(fn, A, C, rhs, CYCLE, alone)

    # the rotated half-box [I; -I[1:]] Q: nothing bounds (Q x)_0 from below, so +Q^T e_0 is UNBOUNDED on every
    # feasible right-hand side; Q^T g with g_0 < 0 is bounded, every (Q x)_j at the end of its interval that g_j picks.
    # Three objectives here: the grids are no multiple of 3, so a workgroup's next program has another objective
    Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
    half = np.vstack([np.eye(N), -np.eye(N)[1:]]) @ Q
    Mh = 2 * N - 1

    def empty(g):
        bad = g.uniform(0.5, 1.5, Mh)
        bad[1], bad[N] = -2.0, 1.0  # (Q x)_1 <= -2 and -(Q x)_1 <= 1
        return bad

    rhs, at_inf, at_nan = _nine_rhs(rng, half, lambda g: g.uniform(0.5, 1.5, Mh), empty)
    G = rng.standard_normal((2, N))
    G[:, 0] = -np.abs(G[:, 0]) - 0.1
    C = np.vstack([Q[:1], G @ Q])
    grid = _grid(kernel, Mh, 3 * R)
    assert 3 * R > grid and grid % 3 != 0
    (obj, status, iters, x), alone = _check_isolation(fn, half, C, rhs, R)
    followed = _followed(status, grid)
    print("LPISOLATION", kernel, "half-box", (Mh, N), "programs", 3 * R, "workgroups", grid, "statuses",
          np.bincount(status.ravel(), minlength=4).tolist(), "iterations", iters.min(), "...", iters.max(),
          "(predecessor, own) statuses", sorted(followed))
    cycle = np.arange(R) % CYCLE
    ok = (cycle != at_inf) & (cycle != at_nan)
    assert np.all(status[ok, 0] == UNB) and np.all(obj[ok, 0] == -np.inf)
    assert np.all(status[ok, 1:] == OPT)
    for k in range(CYCLE):
        if k not in (at_inf, at_nan):
            for o in (1, 2):
                g = G[o - 1]
                exact = g[0] * rhs[k][0] - np.sum(np.abs(g[1:]) * np.where(g[1:] > 0, rhs[k][N:], rhs[k][1:N]))
                assert abs(alone[k, o][0] - exact) <= TOL * max(1.0, abs(exact)), (k, o, alone[k, o][0], exact)
    assert np.all(status[cycle == at_inf] == INF) and np.all(obj[cycle == at_inf] == np.inf)
    assert np.all(status[cycle == at_nan] == NC) and np.all(iters[cycle == at_nan] == 1)
    assert {(UNB, OPT), (OPT, UNB), (INF, OPT), (INF, UNB), (NC, UNB)} <= followed


def test_small_kernel_programs_do_not_depend_on_their_predecessor(eng):
    M, N, R = 7, 3, 1100
    assert 2 * R > 2048 == _grid("small", M, 2 * R)  # more programs than the launch has workgroups
    _isolation(eng, "small", M, N, R)


def test_large_kernel_programs_do_not_depend_on_their_predecessor(eng):
    # LpLarge::ws_doubles(M) = 256 * 256 + 7 M doubles: 528 208 B at M = 70, and 256 MB hold 508 such workgroups (505 at
    # the half-box's M = 129)
    M, N, R = 70, 65, 300
    assert 2 * R > _grid("large", M, 2 * R) == 508 and _grid("large", 2 * N - 1, 3 * R) == 505
    _isolation(eng, "large", M, N, R)


def test_xl_kernel_programs_do_not_depend_on_their_predecessor(eng):
    # one workgroup per compute unit: 256 of them, each with an 8 MB normal matrix that the next program finds as the
    # last one left it, and 48 KB of LDS vectors.  600 and 900 programs on 256 workgroups: 256 is even, 128 is no
    # multiple of CYCLE = 9 and 256 none of 3, as _isolation asks
    M, N, R = 70, 65, 300
    assert 2 * R > _grid("xl", M, 2 * R) == 256 and 3 * R > _grid("xl", 2 * N - 1, 3 * R) == 256
    _isolation(eng, "xl", M, N, R)


@pytest.mark.parametrize("kernel,M,N", [("small", 46, 15), ("small", 193, 64), ("large", 133, 65), ("large", 261, 129),
                                        ("xl", 300, 257)])
def test_nan_in_an_objective_and_in_A(eng, kernel, M, N):
    from quantpy_amd import _capi

    fn = _entry(eng, kernel)
    rng = np.random.default_rng(77 * M + N)
    A, ax0 = lp_cases.bounded_lp(rng, M, N)
    b = ax0[None, :] + rng.uniform(0.01, 1.0, (3, M))
    C = rng.standard_normal((2, N))
    clean = fn(A, C[:1], b, return_x=True)
    assert np.all(clean[1] == _capi.LP_OPTIMAL)
    C[1, N // 2] = np.nan
    obj, status, iters, x = fn(A, C, b, return_x=True)
    assert _same_bits([obj[:, :1], status[:, :1], iters[:, :1], x[:, :1]], clean)
    assert np.all(status[:, 1] == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(obj[:, 1]))
    # a NaN in A: the rank test fails, once per workgroup, and every program says so
    A[M // 3, N - 1] = np.nan
    obj, status, iters = fn(A, C[:1], b)
    assert np.all(status == _capi.LP_NOT_CONVERGED) and np.all(np.isnan(obj)) and np.all(iters == 0)
