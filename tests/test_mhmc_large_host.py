"""The oracle's Metropolis-Hastings chain (mhmc_state_interval) against the reference's n = 4 chains of
tests/golden/mhmc_large.npz: same seed, same sorted distances, acceptance rate and last state.  No GPU."""
import numpy as np
import pytest
from conftest import load_golden


@pytest.mark.parametrize("key", ["L0", "L1"])
def test_oracle_reproduces_reference_chain_n4(oracle, key):
    g = load_golden("mhmc_large")
    n = int(g[key + "_n"])
    assert n == 4
    n_points, burn, thin = (int(v) for v in g[key + "_args"])
    np.random.seed(int(g[key + "_rng_seed"]))
    dist, samples, rate = oracle.mhmc_state_interval(g[key + "_counts"], oracle.measurement_matrix(str(g[key + "_povm"]), n),
                                                     g[key + "_state"], n_points, float(g[key + "_step"]), burn, thin)
    assert np.abs(dist - g[key + "_all_dist"]).max() < 1e-10
    assert rate == float(g[key + "_rate"]) and 0.0 < rate < 1.0
    if thin == 1:  # the last sample is the chain's last state
        assert np.abs(samples[-1] - g[key + "_final_x"]).max() < 1e-12
