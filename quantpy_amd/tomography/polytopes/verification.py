"""`test_qst` / `test_qpt` of the reference (polytopes/verification.py): simulate the tomography `n_trials` times, widen
the measured frequencies by the delta of each confidence level and count how often the true state (process) lies in
the polytope.  The reference does this with one Python `count_delta` per (trial, level); here a chunk of trials is one
launch of qt_polytope_coverage.

The functions are named `test_*` because the reference names them so.  Import the module, not the names, in a pytest
file (they carry `__test__ = False` as a second guard).
"""
import numpy as np

from ...engine import any_engine
from ...sampling import SAMPLERS, draw_counts, resolve_seed, trial_chunks
from ..process import ProcessTomograph
from ..state import StateTomograph

# One launch handles a chunk of trials.  A chunk is bounded by the work of its launch -- trials x levels x 34 bisection
# steps x table entries <= kLaunchEvaluations evaluations of exp(-n KL), which at an estimated 5e10 evaluations per
# second keeps a launch near 0.2 s -- and by the size of its count table (kChunkBytes on the host and on the device).
kLaunchEvaluations = 1e10
kChunkBytes = 128 << 20
_BISECTION_STEPS = 34


def chunk_trials(n_trials, n_entries, n_levels):
    """Trials per launch for tables of `n_entries` counts and `n_levels` confidence levels (at least one)."""
    by_work = kLaunchEvaluations / (_BISECTION_STEPS * max(n_levels, 1) * n_entries)
    by_bytes = kChunkBytes / (8 * n_entries)
    return int(max(1, min(n_trials, by_work, by_bytes)))


def _weighted_povm(povm_matrix, shots):
    """The shot-weighted POVM rows W (verification.py:17-23, :52-55): (S K, 4^n)."""
    return np.reshape(povm_matrix * shots[:, None, None] / np.sum(shots), (-1, povm_matrix.shape[-1])) * povm_matrix.shape[0]


def _run(probas, shots, truth, clip_b, conf_levels, n_trials, sampler, seed, return_table):
    """probas (R, K) outcome distributions, shots (R,), truth (R K,) -> fractions (and hits, deltas)."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, not {sampler!r}")
    levels = np.asarray(conf_levels, dtype=np.float64)
    engine = any_engine()
    if sampler == "numpy":
        # the reference runs one experiment before its loop (verification.py:13-14, :45-46) and one per trial
        draw_counts(shots, probas, 1, "numpy", seed)
    else:
        seed = resolve_seed(seed)
    chunk = chunk_trials(n_trials, probas.size, levels.size)
    covered = np.zeros(levels.size, dtype=np.int64)
    hits, deltas = [], []
    for _, counts in trial_chunks(engine, shots, probas, n_trials, chunk, sampler, seed):
        res = engine.polytope_coverage(counts, shots, levels, truth=truth, clip_b=clip_b, covered=covered,
                                       return_deltas=return_table, return_hits=return_table)
        if return_table:
            covered, d, h = res
            hits.append(h)
            deltas.append(d)
        else:
            covered = res
    fractions = covered / n_trials
    if return_table:
        shape = (0, levels.size)
        return (fractions, np.concatenate(hits) if hits else np.zeros(shape, dtype=bool),
                np.concatenate(deltas) if deltas else np.zeros(shape))
    return fractions


def qst_tables(state, n_measurements, povm="proj-set"):
    """What both state studies are built from: (probas (S, K), shots (S,), W (S K, 4^n), A (S K, 4^n - 1)) -- the outcome
    distributions that feed the sampler, the shots per setting, the shot-weighted POVM rows and the polytope's matrix
    A = W[:, 1:] * d (verification.py:17-23)."""
    povm_matrix, shots, probas = StateTomograph(state)._experiment_tables(n_measurements, povm)
    shots = np.asarray(shots, dtype=np.float64)
    weighted = _weighted_povm(povm_matrix, shots)
    return probas, shots, weighted, np.ascontiguousarray(weighted[:, 1:]) * 2**state.n_qubits


def qpt_tables(channel, n_measurements, input_states="sic", povm="proj-set"):
    """The process counterpart: (probas (D S, K), shots (D S,), W (S K, 4^n), states_matrix (D, 4^n)) from the
    throw-away tomograph's `_experiment_tables` -- row input * S + setting -- and the Bloch vectors of the transposed
    input states (verification.py:43-55)."""
    tmg = ProcessTomograph(channel, input_states=input_states)
    povm_matrix, shots, probas = tmg._experiment_tables(n_measurements, povm)
    shots = np.asarray(shots, dtype=np.float64)
    states_matrix = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements], dtype=np.float64)
    return probas, np.tile(shots, len(states_matrix)), _weighted_povm(povm_matrix, shots), states_matrix


def qst_setup(state, n_measurements, povm="proj-set"):
    """(probas (S, K), shots (S,), truth (S K,)) of test_qst: `qst_tables` and t = A x_true + W[:, 0]
    (verification.py:24-25).  `povm`: the reference uses the default, 'proj-set'; an (S, K, 4^n) array is taken as it
    is."""
    probas, shots, weighted, A = qst_tables(state, n_measurements, povm)
    return probas, shots, A @ np.asarray(state.bloch, dtype=np.float64)[1:] + weighted[:, 0]


def qpt_setup(channel, n_measurements, input_states="sic", povm="proj-set"):
    """(probas (D S, K), shots (D S,), truth (D S K,)) of test_qpt (verification.py:43-60).  The polytope's matrix is
    (input Bloch vectors) (x) (weighted POVM rows), so the true outcome probabilities are a small matrix product; the
    dense (D S K) x (16^n - 4^n) matrix of the reference is never formed."""
    dim = 4**channel.n_qubits
    probas, shots, weighted, states_matrix = qpt_tables(channel, n_measurements, input_states, povm)
    choi = np.asarray(channel.choi.bloch, dtype=np.float64).reshape(dim, dim)[:, 1:]  # indices i with i % dim != 0
    truth = (states_matrix @ choi @ weighted[:, 1:].T) * dim + weighted[None, :, 0]
    return probas, shots, np.ravel(truth)


def test_qst(state, conf_levels, n_measurements=1000, n_trials=1000, *, sampler="numpy", seed=None, return_table=False):
    """Fraction of `n_trials` simulated tomographies of `state` whose polytope at each confidence level holds the state
    (reference verification.py:9-37; default POVM 'proj-set', `n_measurements` shots per setting).

    sampler='numpy' (default): the counts come from np.random's global stream in the reference's order, so
    `np.random.seed(s)` reproduces the reference's run trial for trial and leaves the stream where it leaves it
    (seed must stay None).  sampler='device': the counts are drawn on the GPU from the Philox streams of `seed` (None:
    64 bits of np.random's stream) and never visit the host.  return_table=True: also hits (n_trials, L) bool and
    deltas (n_trials, L)."""
    probas, shots, truth = qst_setup(state, n_measurements)
    return _run(probas, shots, truth, True, conf_levels, n_trials, sampler, seed, return_table)


def test_qpt(channel, conf_levels, n_measurements=1000, n_trials=1000, input_states="sic", *, sampler="numpy", seed=None,
             return_table=False):
    """Fraction of `n_trials` simulated process tomographies of `channel` whose polytope at each confidence level holds
    the channel (reference verification.py:40-78).  The bound is f + delta without the clip of test_qst, as in the
    reference.  Keyword-only arguments: see test_qst."""
    probas, shots, truth = qpt_setup(channel, n_measurements, input_states)
    return _run(probas, shots, truth, False, conf_levels, n_trials, sampler, seed, return_table)


test_qst.__test__ = False
test_qpt.__test__ = False
