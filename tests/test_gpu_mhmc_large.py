"""GPU: MHMCStateInterval at n = 4, 5 qubits (reference interval.py:689-750, mhmc.py) through qt_mhmc_state /
k_mhmc_state_large -- against chains the reference ran (tests/golden/mhmc_large.npz, make_golden_mhmc_large.py), the
oracle's chain state by state, the dense operand path, several chains per launch and the warm start."""
import numpy as np
import pytest
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _tomograph(qp, n, povm, counts, state):
    tmg = qp.StateTomograph(qp.Qobj(np.eye(2**n) / 2**n))
    tmg.experiment(10, povm)
    tmg.results = counts
    tmg.reconstructed_state = qp.Qobj(state)
    return tmg


def _near_basis_state(rng, n):
    d = 2**n
    g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = 0.01 * (g @ g.conj().T) / np.trace(g @ g.conj().T)
    rho[0, 0] += 0.99
    return rho


@pytest.mark.parametrize("key", ["L0", "L1", "L2"])
def test_mhmc_large_matches_reference(qp, key):
    """Same global seed as the reference's run: the radii and every sorted distance to 1e-10, the chain's last state
    (the reference's chain.x_t) to 1e-12 and the acceptance rate exactly.  L2 (n = 5) also pins the direct draw of
    the 1024-dim proposal increments against scipy's frozen multivariate_normal."""
    g = load_golden("mhmc_large")
    n = int(g[key + "_n"])
    n_points, burn, thin = (int(v) for v in g[key + "_args"])
    tmg = _tomograph(qp, n, str(g[key + "_povm"]), g[key + "_counts"], g[key + "_state"])
    np.random.seed(int(g[key + "_rng_seed"]))
    iv = qp.MHMCStateInterval(tmg, n_points=n_points, step=float(g[key + "_step"]), burn_steps=burn, thinning=thin)
    radii = iv(g["conf_levels"])[0]
    assert np.abs(radii - g[key + "_radii"]).max() < 1e-10, (radii, g[key + "_radii"])
    assert np.abs(iv.cl_to_dist(np.linspace(0, 1, n_points)) - g[key + "_all_dist"]).max() < 1e-10
    assert np.abs(iv._x_t - g[key + "_final_x"]).max() < 1e-12
    assert iv.acceptance_rate == float(g[key + "_rate"])
    assert 0.0 < iv.acceptance_rate < 1.0


def _oracle_check(qp, oracle, tmg, state, n_points, step, burn, seed):
    np.random.seed(seed)
    iv = qp.MHMCStateInterval(tmg, n_points=n_points, step=step, burn_steps=burn)
    iv.setup()
    np.random.seed(seed)
    dist, samples, rate = oracle.mhmc_state_interval(tmg.results, oracle.measurement_matrix("proj-set", 4), state,
                                                     n_points, step, burn)
    assert np.abs(iv.samples - samples).max() < 1e-12
    assert np.abs(iv.cl_to_dist(np.linspace(0, 1, n_points)) - dist).max() < 1e-10
    assert iv.acceptance_rate == rate and 0.0 < rate < 1.0
    return iv


def test_mhmc_large_matches_oracle_state_by_state(qp, oracle):
    rho = _near_basis_state(np.random.default_rng(4), 4)
    np.random.seed(40)
    tmg = qp.StateTomograph(qp.Qobj(rho))
    tmg.experiment(1000, "proj-set")
    tmg.reconstructed_state = qp.Qobj(rho)
    _oracle_check(qp, oracle, tmg, rho, 150, 0.5, 50, 404)


def test_mhmc_large_dense_operand_path(qp, oracle):
    """A plain (S, K, 256) array POVM (no one-qubit factor: the dense row_dot_dense path) gives the oracle's chain, and
    the chain of the factorised POVM on the same counts."""
    rho = _near_basis_state(np.random.default_rng(5), 4)
    np.random.seed(50)
    tmg = qp.StateTomograph(qp.Qobj(rho))
    tmg.experiment(1000, "proj-set")
    assert hasattr(tmg.povm_matrix, "valid_factor")
    tmg.reconstructed_state = qp.Qobj(rho)
    prod = _oracle_check(qp, oracle, tmg, rho, 100, 0.5, 40, 505)
    dense = _tomograph(qp, 4, "proj-set", tmg.results, rho)
    dense.povm_matrix = np.array(tmg.povm_matrix)
    assert not hasattr(dense.povm_matrix, "valid_factor")
    iv = _oracle_check(qp, oracle, dense, rho, 100, 0.5, 40, 505)
    assert np.abs(iv.samples - prod.samples).max() < 1e-12
    assert iv.acceptance_rate == prod.acceptance_rate


@pytest.mark.parametrize("n", [4, 5])
def test_mhmc_large_several_chains_per_launch(qp, oracle, n):
    """C = 3 chains on different counts in one launch are bit-identical to three C = 1 launches."""
    povm = qp.generate_measurement_matrix("proj-set", n)
    rng = np.random.default_rng(60 + n)
    states = [_near_basis_state(rng, n) for _ in range(3)]
    np.random.seed(61)
    counts = np.stack([oracle.sample_counts(np.asarray(povm), oracle.bloch_from_matrix(s), 1000) for s in states])
    eng = qp.get_engine(n)
    eng.set_povm(povm, counts[0].sum(-1))
    x0 = np.stack([eng.chol_param(s)[0] for s in states])
    T = 40
    deltas = rng.standard_normal((3, T, 4**n))
    uniforms = rng.random((3, T))
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, 0.5)
    assert chain.shape == (3, T, 4**n) and acc.shape == (3, T)
    for c in range(3):
        ch1, acc1 = eng.mhmc_state(counts[c], x0[c], deltas[c], uniforms[c], 0.5)
        assert np.array_equal(ch1, chain[c]) and np.array_equal(acc1, acc[c])
    assert np.abs(np.linalg.norm(chain, axis=-1) - 1.0).max() < 1e-12
    # a rejected step keeps the state, an accepted one moves it
    prev = np.concatenate([x0[:, None], chain[:, :-1]], axis=1)
    moved = np.any(chain != prev, axis=-1)
    assert np.array_equal(moved, acc.astype(bool))


def test_mhmc_large_warm_start(qp):
    """warm_start at n = 4: the second setup() continues the chain from its last state with no new burn-in -- the same
    samples as one chain of 2 n_points steps after the burn-in."""
    rho = _near_basis_state(np.random.default_rng(7), 4)
    np.random.seed(70)
    tmg = qp.StateTomograph(qp.Qobj(rho))
    tmg.experiment(1000, "proj-set")
    tmg.reconstructed_state = qp.Qobj(rho)
    np.random.seed(707)
    iv = qp.MHMCStateInterval(tmg, n_points=30, step=0.5, burn_steps=20, warm_start=True)
    iv.setup()
    first, last = iv.samples.copy(), iv._x_t.copy()
    iv.setup()
    assert iv._burned and not np.array_equal(last, iv._x_t)
    second = iv.samples.copy()
    # the same draws by hand: burn-in, first 30, then 30 more from where the chain stopped
    from quantpy_amd.tomography.interval import _proposal_increments

    np.random.seed(707)
    jump = _proposal_increments(256)
    draws = [(jump(20), np.random.rand(20)), (jump(30), np.random.rand(30)), (jump(30), np.random.rand(30))]
    eng = tmg._engine()
    x0, _ = eng.chol_param(rho)
    chain, _ = eng.mhmc_state(tmg.results, x0, np.concatenate([d for d, _ in draws]),
                              np.concatenate([u for _, u in draws]), 0.5)
    assert np.array_equal(chain[20:50], first)
    assert np.array_equal(chain[50:80], second)
