"""Shared by tests/test_mhmc_large_coverage_host.py and tests/test_gpu_mhmc_large_coverage.py: the inputs of the chain
coverage study at n = 4, 5 and the yardstick they are run through.

State mixed_ghz(n, 0.5), POVM 'proj-set', three experiments on np.random's stream from seed 100 n + 3 with SHOTS[n] shots
per setting.  At 1000 shots the unclipped 'lin' estimates of these states are not positive definite; at 10 000 (n = 4) and
100 000 (n = 5) their smallest eigenvalues are about 0.020 and 0.012.

STEP = 2.0; settings (burn_steps, n_points, thinning) = (3, 20, 2) and (0, 60, 1).  The reference's target is nearly flat
(about 3 % of the proposals rejected at any step size), so the Philox seeds were found by search on the CPU oracle with the
host build of the draws: the first seeds from 3000 up at which, in both settings, every one of the three chains rejects at
least one post-burn step (and accepts at least one).  Rejected post-burn steps per chain of that run, REJECTED below:
    n = 4, seed 3006: (3, 20, 2) -> [2, 1, 1],  (0, 60, 1) -> [3, 1, 1]
    n = 5, seed 3023: (3, 20, 2) -> [1, 1, 1],  (0, 60, 1) -> [1, 2, 1]
A change of the draws' definition or of the nll arithmetic that moves a marginal step needs a new search."""
import numpy as np

import mhmc_coverage_cases as small

STEP = 2.0
SHOTS = {4: 10_000, 5: 100_000}
CHAINS = 3
SETTINGS = {"thinned": (3, 20, 2), "plain": (0, 60, 1)}  # burn_steps, n_points, thinning
DRAW_SEEDS = {4: 3006, 5: 3023}
REJECTED = {(4, "thinned"): [2, 1, 1], (4, "plain"): [3, 1, 1], (5, "thinned"): [1, 1, 1], (5, "plain"): [1, 2, 1]}
EPS = 2.0**-52


def tol(n):
    """Bound on |fused - unfused| of a distance: FP64 sums of at most d^2 terms of magnitude <= 1, error about d^2 eps,
    times ten (5.7e-13 at n = 4, 2.3e-12 at n = 5)."""
    return 10 * 4**n * EPS


def trial_counts(oracle, n, shots=None):
    """CHAINS experiments on the mixed GHZ state: (counts (C, S, K) int64, the true state)."""
    rho = small.mixed_ghz(n)
    povm = oracle.measurement_matrix("proj-set", n)
    bloch = oracle.bloch_from_matrix(rho)
    np.random.seed(100 * n + 3)
    counts = np.stack([oracle.sample_counts(povm, bloch, SHOTS[n] if shots is None else shots) for _ in range(CHAINS)])
    return counts.astype(np.int64), rho


def smallest_eigenvalues(oracle, n, counts):
    """Of the unclipped 'lin' estimates, on the CPU oracle."""
    povm = oracle.measurement_matrix("proj-set", n)
    return np.array([np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)).min() for c in counts])


def median_off_samples(dist):
    """A threshold in the middle of one chain's distances and on none of them."""
    s = np.unique(dist)
    return 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) > 1 else 1.5 * s[0] + 1e-3


def kept_states(eng, counts, x0, seed, burn, n_points, thinning, step, first_chain=0):
    """The yardstick's chain: qt_mhmc_draws_dim -> qt_mhmc_state -> kept states -> qt_chol_unparam.  Returns (kept
    states (C, n_points, d, d), accepted post-burn steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_draws_dim(eng.D, seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, step)
    chain, acc = chain.reshape(chains, total, eng.D), acc.reshape(chains, total)
    kept = chain[:, burn::thinning][:, :n_points]
    mats = eng.chol_unparam(kept.reshape(-1, eng.D)).reshape(chains, n_points, eng.d, eng.d)
    return mats, acc[:, burn:].sum(axis=1).astype(np.int64)


def unfused_dist(eng, mats, centres, metric):
    """qt_hs_dist_dim (metric None) / qt_metric_dist_dim of the kept states to their chain's centre: (C, n_points)."""
    if metric is None:
        return np.stack([eng.hs_dist(mats[c], centres[c]) for c in range(mats.shape[0])])
    return np.stack([eng.metric_dist_dim(mats[c], centres[c], metric) for c in range(mats.shape[0])])
