"""Shared by tests/test_process_mhmc_large_coverage_host.py and tests/test_gpu_process_mhmc_large_coverage.py: the
three-qubit process tomographies the GPU tests run their chains on.  The first two are those of
test_gpu_batch_positions.n3_processes, the third is built the same way from a third channel."""
import numpy as np

from process_mhmc_coverage_cases import thresholds  # noqa: F401  (re-exported)

N = 3
SHOTS = 10000
STEP = 1e-5  # the step at which test_gpu_batch_positions.py sees about half of a three-qubit chain's proposals accepted
SETTINGS = {"thinned": (2, 5, 2), "plain": (0, 12, 1)}  # burn_steps, n_points, thinning: at most 12 steps
CASES = [1, 3]  # chains: the first tomograph alone, and all three
DIM = 4096  # the vector length of the chain's numbers (qt_mhmc_draws_dim)


def tomographs(qp):
    """(the first tomograph, counts (3, 64, 27, 8) int64): 'proj-set' at SHOTS per setting on the 'proj4' input states.
    POVM, shots and input states are the same for all three, so the first tomograph's engine serves every chain."""
    built = []
    for seed, channel in ((31, qp.channel.depolarizing(0.1, N)),
                          (32, qp.channel.depolarize(qp.channel.walsh_hadamard(N), 0.2)),
                          (33, qp.channel.depolarize(qp.operator.Toffoli.as_channel(), 0.15))):
        np.random.seed(seed)
        tmg = qp.ProcessTomograph(channel)
        tmg.experiment(SHOTS, "proj-set")
        built.append((tmg, channel))
    counts = np.stack([t.results for t, _ in built]).astype(np.int64)
    truths = np.ascontiguousarray(np.stack([c.choi.matrix for _, c in built]))
    assert counts.shape == (3, 64, 27, 8) and len({c.tobytes() for c in counts}) == 3
    return built[0][0], counts, truths
