"""polytopes.StateFidelityIntervalXL / fidelity_qst_xl: the five-qubit polytope programs (7776 x 1023) on
qt_lp_ineq_xl_batch against the reference's PolytopeStateInterval as recorded in tests/golden/polytope5.npz
(make_golden_polytope5.py; the optima there are HiGHS's), the same bits as the names without XL below five qubits, and
the refusal at six."""
import numpy as np
import pytest
from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-9
G = load_golden("polytope5")
NAME = str(G["state_cases"][0])


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def test_five_qubit_interval_against_reference(qp):
    from quantpy_amd import _capi
    from quantpy_amd.tomography.polytopes import StateFidelityIntervalXL

    n, n_points = int(G[NAME + "/n_qubits"]), int(G[NAME + "/n_points"])
    assert (n, n_points) == (5, 2)
    d = 2**n
    tmg = qp.StateTomograph(qp.Qobj(G[NAME + "/true_bloch"]))
    tmg.povm_matrix = qp.generate_measurement_matrix(str(G[NAME + "/povm"]), n)
    tmg.results = G[NAME + "/counts"]
    assert np.array_equal(tmg.n_measurements, G[NAME + "/shots"])
    interval = StateFidelityIntervalXL(tmg, n_points=n_points, target_state=qp.Qobj(G[NAME + "/target_bloch"]))
    interval.setup()
    print("statuses", interval.lp_status.ravel().tolist(), "iterations", interval.lp_iters.ravel().tolist())
    assert np.all(np.abs(interval.deltas - G[NAME + "/deltas"]) <= 1e-12)
    ref_cl = G[NAME + "/conf_levels"]
    assert np.all(np.abs(interval.conf_levels - ref_cl) <= 1e-12 * np.maximum(1.0, np.abs(ref_cl)))
    assert np.all(interval.lp_status == _capi.LP_OPTIMAL) and np.all(interval.lp_iters <= 200)
    assert interval.lp_resolved.all()
    # the objectives, through the bounds 1/d + d obj and 1/d - d obj: the reference's table keeps only the bounds
    ref_obj = G[NAME + "/lp_obj"]
    assert np.all(G[NAME + "/lp_status"] == 0) and np.all(ref_obj != 0.0)
    obj = np.stack([(interval.dist_min - 1 / d) / d, (1 / d - interval.dist_max) / d], axis=1)
    print("objectives", obj.ravel().tolist(), "HiGHS", ref_obj.ravel().tolist(), "largest difference",
          np.abs(obj - ref_obj).max())
    assert np.all(np.abs(obj - ref_obj) <= TOL * np.maximum(1.0, np.abs(ref_obj)))
    for ours, ref, o in ((interval.dist_min, G[NAME + "/dist_min"], 0), (interval.dist_max, G[NAME + "/dist_max"], 1)):
        assert np.all(np.abs(ours - ref) <= d * TOL * np.maximum(1.0, np.abs(ref_obj[:, o])))
    # the true state lies in the wider polytope, so its fidelity lies within that widening's bounds
    fid = float(d * (G[NAME + "/target_bloch"] @ G[NAME + "/true_bloch"]))
    assert interval.dist_min[-1] <= fid + 1e-9 and interval.dist_max[-1] >= fid - 1e-9


def test_xl_interval_is_state_fidelity_interval_at_two_qubits(qp):
    from quantpy_amd.tomography.polytopes import StateFidelityInterval, StateFidelityIntervalXL

    rng = np.random.default_rng(18)
    g = rng.standard_normal((4, 4)) + 1j * rng.standard_normal((4, 4))
    rho = g @ g.conj().T
    tmg = qp.StateTomograph(qp.Qobj(rho / np.trace(rho)))
    np.random.seed(42)
    tmg.experiment(1000)
    old = StateFidelityInterval(tmg, n_points=40)
    new = StateFidelityIntervalXL(tmg, n_points=40)
    old.setup()
    new.setup()
    for attr in ("deltas", "conf_levels", "dist_min", "dist_max", "lp_status", "lp_iters", "lp_resolved"):
        assert np.array_equal(getattr(old, attr), getattr(new, attr)), attr


def test_fidelity_qst_xl_at_five_qubits(qp):
    from quantpy_amd import _capi
    from quantpy_amd.tomography.polytopes import fidelity_qst_xl

    target = qp.qobj.GHZ(5)
    state = qp.channel.depolarizing(0.1, 5).transform(target)
    runs = [fidelity_qst_xl(state, target, [0.9], 1000, 1, sampler="device", seed=11, return_table=True, chunk=chunk)
            for chunk in (None, 1)]
    f_min, f_max, table = runs[0]
    print("f_min", f_min, "f_max", f_max, "iterations", table["lp_iters"].ravel().tolist())
    assert f_min.shape == f_max.shape == (1, 1)
    assert np.all(table["lp_status"] == _capi.LP_OPTIMAL) and table["lp_resolved"].all()
    assert np.isfinite(f_min).all() and np.isfinite(f_max).all() and f_min[0, 0] <= f_max[0, 0]
    assert np.array_equal(f_min, runs[1][0]) and np.array_equal(f_max, runs[1][1])
    for key in ("deltas", "lp_status", "lp_iters", "lp_resolved"):
        assert np.array_equal(table[key], runs[1][2][key]), key


def test_launch_split_changes_no_bit(qp, monkeypatch):
    """_lp_in_launches over several launches (the cap lowered to two programs) against one launch."""
    import lp_xl_cases as cases
    from quantpy_amd import get_engine
    from quantpy_amd.tomography.polytopes import fidelity

    eng = get_engine(1)
    A, C, b = cases.random_batch(300, 256, 3)
    whole = fidelity._lp_in_launches(eng, A, C, b)
    monkeypatch.setattr(fidelity, "kLaunchProgramsXL", 2)
    split = fidelity._lp_in_launches(eng, A, C, b)
    assert all(np.array_equal(u, v) for u, v in zip(whole[0], split[0])) and np.array_equal(whole[1], split[1])
    assert all(np.array_equal(u, v) for u, v in zip(whole[0], eng.lp_ineq_xl_batch(A, C, b)))


def test_six_qubits_are_refused(qp):
    from quantpy_amd.tomography.polytopes import StateFidelityIntervalXL, fidelity_qst_xl

    t6 = qp.StateTomograph(qp.qobj.fully_mixed(6))
    with pytest.raises(NotImplementedError, match="n <= 5"):
        StateFidelityIntervalXL(t6, n_points=2).setup()
    with pytest.raises(NotImplementedError, match="n <= 5"):
        fidelity_qst_xl(qp.qobj.fully_mixed(6), qp.qobj.fully_mixed(6), [0.9], n_trials=1)
