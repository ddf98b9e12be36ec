"""quantpy_amd.tomography.polytopes.fidelity: ProcessFidelityInterval / StateFidelityInterval against the reference's
PolytopeProcessInterval (n = 1, 2) and PolytopeStateInterval (n = 4) as recorded in tests/golden/polytope_fidelity.npz
(make_golden_polytope_fidelity.py; the optima there are HiGHS's), and the study functions fidelity_qpt / fidelity_qst
against the host count_delta and HiGHS."""
import numpy as np
import polytope_fidelity_cases as cases
import pytest
from scipy.interpolate import interp1d
from scipy.optimize import linprog

pytestmark = pytest.mark.gpu

G = cases.golden()


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _highs(c, A, b):
    return linprog(c, A_ub=A, b_ub=b, bounds=[(None, None)] * A.shape[1], method="highs")


def _process_interval(qp, name):
    from quantpy_amd.tomography.polytopes import ProcessFidelityInterval

    n = int(G[name + "/n_qubits"])
    p_true, p_target = G[name + "/depolarizing"]
    channel, target = qp.channel.depolarizing(p_true, n), qp.channel.depolarizing(p_target, n)
    assert np.abs(channel.choi.bloch - G[name + "/true_bloch"]).max() < 1e-14
    tmg = qp.ProcessTomograph(channel, input_states=str(G[name + "/input_states"]))
    povm = qp.generate_measurement_matrix(str(G[name + "/povm"]), n)
    tmg.tomographs = [qp.StateTomograph(channel.transform(rho)) for rho in tmg.input_basis.elements]
    for t, counts in zip(tmg.tomographs, G[name + "/counts"]):
        t.povm_matrix, t.results, t.n_measurements = povm, counts, G[name + "/shots"]
    return ProcessFidelityInterval(tmg, n_points=int(G[name + "/n_points"]), target_channel=target), channel, target


def _state_interval(qp, name, cls=None):
    from quantpy_amd.tomography.polytopes import StateFidelityInterval

    n = int(G[name + "/n_qubits"])
    tmg = qp.StateTomograph(qp.Qobj(G[name + "/true_bloch"]))
    tmg.povm_matrix = qp.generate_measurement_matrix(str(G[name + "/povm"]), n)
    tmg.results = G[name + "/counts"]
    target = qp.Qobj(G[name + "/target_bloch"])
    return (cls or StateFidelityInterval)(tmg, n_points=int(G[name + "/n_points"]), target_state=target)


def _check_against_fixture(interval, name):
    from quantpy_amd import _capi

    interval.setup()
    n_points = int(G[name + "/n_points"])
    lo_d, hi_d = G[name + "/delta_range"]
    assert np.array_equal(interval.deltas, np.linspace(lo_d, hi_d, n_points))
    ref_cl = G[name + "/conf_levels"]
    assert np.all(np.abs(interval.conf_levels - ref_cl) <= 1e-15 * np.abs(ref_cl))
    A, b, c, _, _ = interval.programs()
    assert A.shape == tuple(G[name + "/G_shape"])
    assert np.array_equal(A[G[name + "/G_rows"]], G[name + "/G_sample"])
    assert abs(A.sum() - G[name + "/G_sum"]) <= 1e-12 * np.abs(A).sum()
    assert abs((A * A).sum() - G[name + "/G_sumsq"]) <= 1e-12 * G[name + "/G_sumsq"]
    assert np.array_equal(c, G[name + "/c"]) and np.array_equal(b[G[name + "/h_rows"]], G[name + "/h"])
    print(name, "statuses", np.unique(interval.lp_status).tolist(), "iterations", int(interval.lp_iters.min()),
          int(interval.lp_iters.max()))
    assert not np.any(interval.lp_status == _capi.LP_NOT_CONVERGED)
    assert np.array_equal(interval.lp_status == _capi.LP_INFEASIBLE, G[name + "/lp_status"] == 2)
    assert np.all(interval.lp_iters <= 200)
    print(name, "largest difference of a bound", np.abs(interval.dist_min - G[name + "/dist_min"]).max(),
          np.abs(interval.dist_max - G[name + "/dist_max"]).max())
    assert np.abs(interval.dist_min - G[name + "/dist_min"]).max() <= 1e-8
    assert np.abs(interval.dist_max - G[name + "/dist_max"]).max() <= 1e-8
    levels = np.linspace(max(1e-3, ref_cl.min()), min(1 - 1e-3, ref_cl.max()), 23)
    (lo, hi), cl = interval(levels)
    assert np.array_equal(cl, levels)
    assert np.array_equal(lo, interp1d(interval.conf_levels, interval.dist_min)(levels))
    assert np.array_equal(hi, interp1d(interval.conf_levels, interval.dist_max)(levels))
    return A, b, c


@pytest.mark.parametrize("name", list(G["process_cases"]))
def test_process_interval_against_reference(qp, name):
    interval, channel, target = _process_interval(qp, name)
    n = int(G[name + "/n_qubits"])
    A, b, c = _check_against_fixture(interval, name)
    # containment: wherever the true Choi vector lies in the polytope, the true fidelity lies within the bounds
    dim = 4**n
    x_true = G[name + "/true_bloch"].reshape(dim, dim)[:, 1:].ravel()
    fid = float(G[name + "/target_bloch"] @ G[name + "/true_bloch"])
    assert abs(1 / dim + c @ x_true - fid) < 1e-12
    inside = np.all(A @ x_true <= b + 1e-12, axis=1)
    assert inside.any()
    assert np.all(interval.dist_min[inside] <= fid + 1e-9) and np.all(interval.dist_max[inside] >= fid - 1e-9)


@pytest.mark.parametrize("name", list(G["state_cases"]))
def test_state_interval_at_four_qubits_against_reference(qp, name):
    interval = _state_interval(qp, name)
    A, b, c = _check_against_fixture(interval, name)
    d = 2 ** int(G[name + "/n_qubits"])
    x_true = G[name + "/true_bloch"][1:]
    fid = 1 / d + d * (c @ x_true)
    inside = np.all(A @ x_true <= b + 1e-12, axis=1)
    assert inside.any()
    assert np.all(interval.dist_min[inside] <= fid + 1e-9) and np.all(interval.dist_max[inside] >= fid - 1e-9)


def test_state_fidelity_interval_is_polytope_state_interval_up_to_three_qubits(qp):
    from quantpy_amd.tomography.polytopes import StateFidelityInterval

    rng = np.random.default_rng(17)
    for n, n_points in ((1, 60), (2, 40), (3, 12)):
        d = 2**n
        g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
        rho = g @ g.conj().T
        tmg = qp.StateTomograph(qp.Qobj(rho / np.trace(rho)))
        np.random.seed(40 + n)
        tmg.experiment(1000)
        old = qp.PolytopeStateInterval(tmg, n_points=n_points)
        new = StateFidelityInterval(tmg, n_points=n_points)
        old.setup()
        new.setup()
        for attr in ("deltas", "conf_levels", "dist_min", "dist_max", "lp_status", "lp_iters"):
            assert np.array_equal(getattr(old, attr), getattr(new, attr)), attr


def test_small_programs_the_small_kernel_leaves_are_solved_by_the_large_one(qp):
    """A pure target (GHZ) makes the optimum degenerate: k_lp_ineq's plain Cholesky breaks down on some widenings of the
    two-qubit state polytope (15 variables).  Those right-hand sides, and only those, carry the large kernel's results,
    x included, and are marked."""
    from quantpy_amd import _capi, get_engine
    from quantpy_amd.tomography.polytopes import StateFidelityInterval

    target = qp.qobj.GHZ(2)
    tmg = qp.StateTomograph(qp.channel.depolarizing(0.1, 2).transform(target))
    np.random.seed(102)
    tmg.experiment(1000)
    interval = StateFidelityInterval(tmg, n_points=40, target_state=target)
    interval.setup()
    A, b, c, _, _ = interval.programs()
    C = np.stack([c, -c])
    eng = get_engine(2)
    small = eng.lp_ineq_batch(A, C, b, return_x=True)
    left = (small[1] == _capi.LP_NOT_CONVERGED).any(axis=1)
    print("right-hand sides the small kernel leaves:", int(left.sum()), "of", left.size)
    assert left.any()  # otherwise this test covers nothing: pick other counts
    picked, resolved = eng._lp_ineq_by_size(A, C, b, return_x=True)
    assert np.array_equal(resolved, left) and np.array_equal(interval.lp_resolved, left)
    large = eng.lp_ineq_large_batch(A, C, b[left], return_x=True)
    for got, s, l in zip(picked, small, large):
        assert np.array_equal(got[~left], s[~left]) and np.array_equal(got[left], l)
    assert np.all(picked[1] == _capi.LP_OPTIMAL)
    assert np.array_equal(interval.lp_status, picked[1]) and np.array_equal(interval.lp_iters, picked[2])
    for r in np.flatnonzero(left)[:6]:
        for o in range(2):
            ref = _highs(C[o], A, b[r])
            assert ref.status == 0 and abs(picked[0][r, o] - ref.fun) <= 1e-9 * max(1.0, abs(ref.fun))
            assert np.all(A @ picked[3][r, o] <= b[r] + 1e-9)
    # the old class, on the small kernel alone, refuses this tomograph
    with pytest.raises(RuntimeError, match="did not converge"):
        qp.PolytopeStateInterval(tmg, n_points=40, target_state=target).setup()


def _study_programs(qp, kind, n):
    """The (A, offset, c, clip, scale, base) of fidelity_qpt / fidelity_qst, from the package's own host pieces."""
    from quantpy_amd.tomography.polytopes import fidelity, verification

    if kind == "process":
        dim = 4**n
        channel, target = qp.channel.depolarizing(0.1, n), qp.channel.depolarizing(0, n)
        tmg = qp.ProcessTomograph(channel, input_states="sic")
        povm = qp.generate_measurement_matrix("proj-set", n)
        shots = np.full(povm.shape[0], 1000.0)
        weighted = verification._weighted_povm(povm, shots)
        states = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements])
        A = fidelity.process_matrix(states, weighted, dim)
        c = target.choi.bloch.reshape(dim, dim)[:, 1:].ravel()
        probas, all_shots, _ = verification.qpt_setup(channel, 1000, "sic")
        return (channel, target), A, np.tile(weighted[:, 0], len(states)), c, False, 1.0, 1 / dim, probas, all_shots
    d = 2**n
    target = qp.qobj.GHZ(n)
    state = qp.channel.depolarizing(0.1, n).transform(target)
    povm = qp.generate_measurement_matrix("proj-set", n)
    shots = np.full(povm.shape[0], 1000.0)
    weighted = verification._weighted_povm(povm, shots)
    A = np.ascontiguousarray(weighted[:, 1:]) * d
    probas, all_shots, _ = verification.qst_setup(state, 1000)
    return (state, target), A, weighted[:, 0], target.bloch[1:], True, float(d), 1 / d, probas, all_shots


LEVELS = [0.5, 0.9, 0.99, 0.999]


@pytest.mark.parametrize("kind,n", [("process", 1), ("process", 2), ("state", 2), ("state", 4)])
def test_fidelity_study_against_host_delta_and_highs(qp, kind, n):
    from quantpy_amd import _capi
    from quantpy_amd.sampling import draw_counts
    from quantpy_amd.tomography.interval import count_delta
    from quantpy_amd.tomography.polytopes import fidelity_qpt, fidelity_qst

    (true, target), A, offset, c, clip, scale, base, probas, shots = _study_programs(qp, kind, n)
    run = fidelity_qpt if kind == "process" else fidelity_qst
    np.random.seed(100 + n)
    f_min, f_max, table = run(true, target, LEVELS, n_measurements=1000, n_trials=3, return_table=True)
    assert f_min.shape == f_max.shape == (3, 4) and table["lp_status"].shape == (3, 4, 2)
    print(kind, n, "iterations", int(table["lp_iters"].min()), int(table["lp_iters"].max()))
    assert np.all(table["lp_status"] == _capi.LP_OPTIMAL) and np.all(table["lp_iters"] <= 200)
    assert table["lp_resolved"].shape == (3, 4) and (A.shape[1] <= 64 or table["lp_resolved"].all())
    # the same counts from the same stream: one experiment before the loop, then one per trial
    np.random.seed(100 + n)
    draw_counts(shots, probas, 1, "numpy", None)
    counts = draw_counts(shots, probas, 3, "numpy", None)
    freq = np.clip(counts / shots[None, :, None], 1e-15, 1 - 1e-15)
    for t in range(3):
        for l, level in enumerate(LEVELS):
            host = count_delta(level, freq[t], shots)
            assert abs(table["deltas"][t, l] - host) <= 2.5e-10
            b = np.ravel(freq[t]) + table["deltas"][t, l]
            b = (np.clip(b, 1e-15, 1 - 1e-15) if clip else b) - offset
            lo, hi = _highs(c, A, b), _highs(-c, A, b)
            assert lo.status == 0 and hi.status == 0
            print(kind, n, t, l, "min", f_min[t, l], base + scale * lo.fun, "max", f_max[t, l], base - scale * hi.fun)
            assert abs(f_min[t, l] - (base + scale * lo.fun)) <= 1e-9 * scale * max(1.0, abs(lo.fun))
            assert abs(f_max[t, l] - (base - scale * hi.fun)) <= 1e-9 * scale * max(1.0, abs(hi.fun))
    assert np.all(f_min <= f_max)
    # the chunking does not change a number
    for chunk in (1, 2):
        np.random.seed(100 + n)
        again = run(true, target, LEVELS, n_measurements=1000, n_trials=3, return_table=True, chunk=chunk)
        assert np.array_equal(again[0], f_min) and np.array_equal(again[1], f_max)
        assert all(np.array_equal(again[2][k], table[k]) for k in table)


@pytest.mark.parametrize("kind,n", [("process", 1), ("state", 2)])
def test_fidelity_study_device_sampler_is_reproducible(qp, kind, n):
    from quantpy_amd.tomography.polytopes import fidelity_qpt, fidelity_qst

    (true, target) = _study_programs(qp, kind, n)[0]
    run = fidelity_qpt if kind == "process" else fidelity_qst
    first = run(true, target, LEVELS, n_trials=5, sampler="device", seed=77, return_table=True)
    second = run(true, target, LEVELS, n_trials=5, sampler="device", seed=77, return_table=True, chunk=2)
    other = run(true, target, LEVELS, n_trials=5, sampler="device", seed=78)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    assert all(np.array_equal(first[2][k], second[2][k]) for k in first[2])
    assert np.all(np.isfinite(first[0])) and np.all(first[0] <= first[1])
    assert not np.array_equal(first[0], other[0])
    with pytest.raises(ValueError, match="sampler"):
        run(true, target, LEVELS, n_trials=1, sampler="cpu")


def test_limits_and_pinned_refusals(qp):
    from quantpy_amd import _capi, get_engine
    from quantpy_amd.engine import EngineError
    from quantpy_amd.tomography.polytopes import (ProcessFidelityInterval, StateFidelityInterval, fidelity_qpt,
                                                  fidelity_qst)

    # what this module does not do
    proc3 = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
    proc3.experiment(10)
    with pytest.raises(NotImplementedError, match="n <= 2"):
        ProcessFidelityInterval(proc3, n_points=4).setup()
    with pytest.raises(NotImplementedError, match="n <= 2"):
        fidelity_qpt(qp.channel.depolarizing(0.1, 3), qp.channel.depolarizing(0, 3), [0.9], n_trials=1)
    t5 = qp.StateTomograph(qp.qobj.fully_mixed(5))
    t5.experiment(10)
    with pytest.raises(NotImplementedError, match="n <= 4"):
        StateFidelityInterval(t5, n_points=4).setup()
    with pytest.raises(NotImplementedError, match="n <= 4"):
        fidelity_qst(qp.qobj.fully_mixed(5), qp.qobj.fully_mixed(5), [0.9], n_trials=1)
    t1 = qp.StateTomograph(qp.qobj.fully_mixed(1))
    t1.experiment(100)
    with pytest.raises(NotImplementedError, match="process tomography"):
        ProcessFidelityInterval(t1)
    proc1 = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 1), input_states="sic")
    with pytest.raises(NotImplementedError, match="state tomography"):
        StateFidelityInterval(proc1)
    # a POVM that is not informationally complete raises before any launch
    proc1.experiment(100, np.array([[[0.5, 0, 0, 0.5], [0.5, 0, 0, -0.5]]]))
    with pytest.raises(ValueError, match="Rank"):
        ProcessFidelityInterval(proc1, n_points=4).setup()
    # the three refusals that existing tests pin stay refusals
    ptm = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 1))
    ptm.experiment(100)
    with pytest.raises(NotImplementedError, match="ProcessFidelityInterval"):
        qp.PolytopeProcessInterval(ptm)
    with pytest.raises(NotImplementedError):
        qp.MomentFidelityProcessInterval(ptm)
    t4 = qp.StateTomograph(qp.qobj.fully_mixed(4))
    t4.experiment(100)
    with pytest.raises(NotImplementedError, match="n <= 3"):
        qp.PolytopeStateInterval(t4, n_points=10).setup()
    rng = np.random.default_rng(5)
    with pytest.raises(EngineError) as err:
        get_engine(1).lp_ineq_batch(rng.standard_normal((70, 65)), np.ones((1, 65)), np.ones((1, 70)))
    assert err.value.code == _capi.QT_ERR_UNSUPPORTED
