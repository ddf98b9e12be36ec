"""Fidelity bounds from the confidence polytope (Kiktenko et al., arXiv:2109.04734, section on fidelity and Fig. 2a):
the reference's `PolytopeProcessInterval` (interval.py:338-418) and the study "Multiple intervals for fidelity" of
polytopes/notebooks/Fidelity.ipynb, with every linear program of a call in one launch of the batched interior-point
solver -- qt_lp_ineq_batch up to 64 variables, qt_lp_ineq_large_batch up to 255 (a two-qubit process has 240, a
four-qubit state 255), qt_lp_ineq_xl_batch up to 1023 (a five-qubit state).

`ProcessFidelityInterval` and `StateFidelityInterval` are the interval classes (one tomograph, n_points widenings);
`fidelity_qpt` and `fidelity_qst` simulate many tomographs and bound the fidelity of each at given confidence levels.
`StateFidelityIntervalXL` and `fidelity_qst_xl` are the state versions up to five qubits (the names without XL keep
their limit of four).
`quantpy_amd.PolytopeProcessInterval` stays the reference's placeholder and `PolytopeStateInterval` keeps its limit of
three qubits; the classes here are the ones to use.
"""
import numpy as np
from ... import _capi
from ...engine import any_engine, get_engine
from ...sampling import SAMPLERS, draw_counts, resolve_seed, trial_chunks
from ..interval import ConfidenceInterval, Mode, PolytopeStateInterval, _FidelityBounds, _pop_hidden_keys, count_delta
from .verification import _weighted_povm, chunk_trials, qpt_tables, qst_tables

__all__ = ["ProcessFidelityInterval", "StateFidelityInterval", "StateFidelityIntervalXL", "fidelity_qpt", "fidelity_qst",
           "fidelity_qst_xl", "process_matrix", "process_programs"]

# Programs per launch of the study functions: a program of the large kernel occupies a workgroup for milliseconds
# (DESIGN 4.8), one of the small kernel for tens of microseconds; both bounds keep a launch well under a second.  A
# program of the XL kernel (above 255 variables) occupies a compute unit for 3.7 s at 7776 x 1023 (measured:
# profiles/lp_xl_timing.txt), and the grid has 256 workgroups: one program each, so that a launch ends with its first
# wave of programs (5.0 s for 256 of them).
kLaunchProgramsSmall = 1 << 16
kLaunchProgramsLarge = 1 << 12
kLaunchProgramsXL = 256
kRhsBytes = 128 << 20


def _launch_cap(n_variables):
    return kLaunchProgramsSmall if n_variables <= 64 else kLaunchProgramsLarge if n_variables <= 255 else kLaunchProgramsXL


def _lp_in_launches(engine, A, C, b):
    """engine._lp_ineq_by_size(A, C, b); above 255 variables in launches of at most kLaunchProgramsXL programs (whole
    right-hand sides).  The programs are independent, so the split changes no bit."""
    per = max(1, kLaunchProgramsXL // len(C))
    if A.shape[1] <= 255 or len(b) <= per:
        return engine._lp_ineq_by_size(A, C, b)
    parts = [engine._lp_ineq_by_size(A, C, b[i:i + per]) for i in range(0, len(b), per)]
    return tuple(np.concatenate([p[0][k] for p in parts]) for k in range(3)), np.concatenate([p[1] for p in parts])


def process_matrix(states_matrix, weighted, dim):
    """A = (input Bloch vectors) (x) (weighted POVM rows[:, 1:]) * dim, rows (input, setting, outcome), columns the
    Choi Bloch indices i with i % dim_out^2 != 0 (reference interval.py:383-386)."""
    meas = np.ascontiguousarray(weighted[:, 1:])
    A = np.einsum("ia,jb->ijab", states_matrix, meas) * dim
    return np.ascontiguousarray(A.reshape(states_matrix.shape[0] * meas.shape[0], -1))


def _require_full_rank(A):
    if np.linalg.matrix_rank(A) < A.shape[1]:
        raise ValueError("Rank(A) < size(x): the measurements are not informationally complete")


def process_programs(states_matrix, povm_matrix, shots, counts, n_points, eps=1e-15):
    """The constraints of the reference's process LPs (interval.py:370-399) from plain arrays: states_matrix (D, 4^n)
    Bloch vectors of the transposed input states, povm_matrix (S, K, 4^n), shots (S,), counts (D, S, K) ->
    (A (D S K, 16^n - 4^n), b (n_points, D S K), deltas, frequencies (D, S, K)).  b = f + delta - tile(W[:, 0]), not
    clipped; the shots of the first output tomograph stand for all, as in the reference."""
    shots = np.asarray(shots, dtype=np.float64)
    states_matrix = np.asarray(states_matrix, dtype=np.float64)
    frequencies = np.clip(np.asarray(counts) / shots[:, None], eps, 1 - eps)
    weighted = _weighted_povm(np.asarray(povm_matrix, dtype=np.float64), shots)
    A = process_matrix(states_matrix, weighted, states_matrix.shape[1])
    _require_full_rank(A)
    deltas = np.linspace(count_delta(0, frequencies, shots), count_delta(1 - 1e-7, frequencies, shots), n_points)
    b = np.ravel(frequencies)[None, :] + deltas[:, None] - np.tile(weighted[:, 0], len(states_matrix))[None, :]
    return A, b, deltas, frequencies


class StateFidelityInterval(PolytopeStateInterval):
    """`PolytopeStateInterval` up to four qubits: the same programs (its `programs()`), solved by the LP kernel that the
    number of variables asks for.  At n <= 3 that is the kernel of PolytopeStateInterval and the results are its
    results bit for bit; at n = 4 (255 variables) it is qt_lp_ineq_large_batch.  Where PolytopeStateInterval raises
    because a program did not converge (a pure target such as GHZ makes the optimum degenerate and the small kernel's
    Cholesky break down), this class solves those widenings with the large kernel instead; `lp_resolved` (n_points,)
    bool marks the widenings whose `lp_status` / `lp_iters` are the large kernel's."""

    _MAX_QUBITS, _MAX_VARIABLES = 4, 255

    def _lp(self, A, C, b):
        res, self.lp_resolved = get_engine(self.tmg.state.n_qubits)._lp_ineq_by_size(A, C, b)
        return res


class StateFidelityIntervalXL(StateFidelityInterval):
    """`StateFidelityInterval` up to five qubits.  At n <= 4 it is that class, bit for bit; at n = 5 (1023 variables, A
    is 7776 x 1023 with 'proj-set') the programs run on qt_lp_ineq_xl_batch, in launches of kLaunchProgramsXL programs:
    the default n_points = 1000 is eight launches of 5 s each (36 s measured for the whole setup(),
    profiles/lp_xl_timing.txt)."""

    _MAX_QUBITS, _MAX_VARIABLES = 5, 1023

    def _lp(self, A, C, b):
        res, self.lp_resolved = _lp_in_launches(get_engine(self.tmg.state.n_qubits), A, C, b)
        return res


class ProcessFidelityInterval(_FidelityBounds, ConfidenceInterval):
    """Fidelity bounds with a target channel from the polytope of a process tomography (reference
    PolytopeProcessInterval, interval.py:338-418), n = 1 and 2 qubits.

    The variables are the Choi Bloch components i with i % dim_out^2 != 0 (the others are fixed by trace
    preservation); A x <= b(delta) with A = process_matrix(...), b = f + delta - tile(W[:, 0]) -- without the clip of the
    state interval, as in the reference -- for n_points widenings between count_delta(0) and count_delta(1 - 1e-7).  The
    bounds at confidence level count_confidence(delta) are 1/dim + min c . x and 1/dim - min(-c . x), dim = 4^n,
    c = target.choi.bloch at those indices.  A missing optimum and an optimum of exactly 0.0 give 1, as in the
    reference; a program that does not converge raises; a rank-deficient A raises ValueError before any launch."""

    def __init__(self, tmg, n_points=1000, target_channel=None):
        super().__init__(tmg, **_pop_hidden_keys(locals()))
        if self.mode != Mode.CHANNEL:
            raise NotImplementedError("ProcessFidelityInterval works only for process tomography")

    def programs(self):
        """(A, b (n_points, M), c, deltas, frequencies (D, S, K)) of the reference's LPs (interval.py:362-400)."""
        tmg = self.tmg
        n_qubits = tmg.channel.n_qubits
        if n_qubits > 2:
            raise NotImplementedError(f"ProcessFidelityInterval supports n <= 2 qubits (16^n - 4^n <= 255 LP variables); "
                                      f"got n = {n_qubits}")
        dim = 4**n_qubits
        first = tmg.tomographs[0]
        states_matrix = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements], dtype=np.float64)
        A, b, deltas, frequencies = process_programs(states_matrix, first.povm_matrix, first.n_measurements,
                                                     [t.results for t in tmg.tomographs], self.n_points)
        target = tmg.channel if self.target_channel is None else self.target_channel
        c = np.asarray(target.choi.bloch, dtype=np.float64).reshape(dim, dim)[:, 1:].ravel()
        return A, b, c, deltas, frequencies

    def setup(self):
        tmg = self.tmg
        if self.target_channel is None:
            self.target_channel = tmg.channel
        dim = 4**tmg.channel.n_qubits
        A, b, c, deltas, frequencies = self.programs()
        engine = get_engine(tmg.channel.n_qubits)
        lp, self.lp_resolved = engine._lp_ineq_by_size(A, np.stack([c, -c]), b)
        self._tabulate_polytope(lp, deltas, frequencies, tmg.tomographs[0].n_measurements, lambda v: 1 / dim + v,
                                lambda v: 1 / dim - v)


def _study(probas, shots, A, offset, c, scale, base, clip_b, conf_levels, n_trials, sampler, seed, return_table, chunk):
    """The figure-2a loop: counts and deltas as in verification._run, then the two programs of every (trial, level) of a
    chunk in one LP launch.  Bounds base + scale * obj and base - scale * obj; NaN where a program is not optimal."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, not {sampler!r}")
    _require_full_rank(A)
    levels = np.atleast_1d(np.asarray(conf_levels, dtype=np.float64))
    n_rows, n_out = probas.shape
    n_lv, m = levels.size, A.shape[0]
    engine = any_engine()
    if sampler == "numpy":
        draw_counts(shots, probas, 1, "numpy", seed)  # the notebook runs one experiment before its loop
    else:
        seed = resolve_seed(seed)
    if chunk is None:
        chunk = min(chunk_trials(n_trials, n_rows * n_out, n_lv), _launch_cap(A.shape[1]) // (2 * max(n_lv, 1)),
                    kRhsBytes // (8 * m * max(n_lv, 1)))
    chunk = int(max(1, min(chunk, max(n_trials, 1))))
    C = np.stack([c, -c])
    f_min = np.full((n_trials, n_lv), np.nan)
    f_max = np.full((n_trials, n_lv), np.nan)
    deltas = np.zeros((n_trials, n_lv))
    status = np.zeros((n_trials, n_lv, 2), dtype=np.int32)
    iters = np.zeros((n_trials, n_lv, 2), dtype=np.int32)
    resolved = np.zeros((n_trials, n_lv), dtype=bool)
    shots_rows = np.asarray(shots, dtype=np.float64)[:, None]
    for start, counts in trial_chunks(engine, shots, probas, n_trials, chunk, sampler, seed):
        size = counts.shape[0]
        dl = engine.polytope_coverage(counts, shots, levels, return_deltas=True)
        if sampler == "device":
            counts = counts.cpu().numpy()
        if n_lv == 0:
            continue
        freq = np.clip(counts.reshape(size, n_rows, n_out) / shots_rows, 1e-15, 1 - 1e-15).reshape(size, 1, m)
        b = freq + dl[:, :, None]
        if clip_b:
            b = np.clip(b, 1e-15, 1 - 1e-15)
        b = (b - offset).reshape(size * n_lv, m)
        (obj, st, it), large = _lp_in_launches(engine, A, C, b)
        sl = slice(start, start + size)
        obj = np.where(st == _capi.LP_OPTIMAL, obj, np.nan).reshape(size, n_lv, 2)
        lo, hi = base + scale * obj[..., 0], base - scale * obj[..., 1]
        both = np.isfinite(lo) & np.isfinite(hi)
        f_min[sl], f_max[sl] = np.where(both, lo, np.nan), np.where(both, hi, np.nan)
        deltas[sl], status[sl], iters[sl] = dl, st.reshape(size, n_lv, 2), it.reshape(size, n_lv, 2)
        resolved[sl] = large.reshape(size, n_lv)
    if return_table:
        return f_min, f_max, {"deltas": deltas, "lp_status": status, "lp_iters": iters, "lp_resolved": resolved}
    return f_min, f_max


def fidelity_qst(state, target_state, conf_levels, n_measurements=1000, n_trials=100, *, sampler="numpy", seed=None,
                 return_table=False, chunk=None):
    """Fidelity bounds of `n_trials` simulated tomographies of `state` ('proj-set', `n_measurements` shots per setting)
    with `target_state` at each confidence level: delta = count_delta(level) per (trial, level) on the GPU, then
    1/d + d min c . x and 1/d - d min(-c . x) over the polytope A x <= clip(f + delta) - W[:, 0] (the programs of
    StateFidelityInterval; n <= 4).  -> (f_min, f_max), each (n_trials, L); NaN in both where one of the two programs
    is not optimal (no mapping to 1 here).  return_table=True adds a dict with `deltas` (n_trials, L), `lp_status` and
    `lp_iters` (n_trials, L, 2) and `lp_resolved` (n_trials, L) bool: True where the programs were solved by the large
    kernel (always above 64 variables; below, where the small kernel left one NOT_CONVERGED).  sampler / seed: as
    verification.test_qst.  chunk: trials per launch (default: bounded by the work and the memory of a launch); the
    results do not depend on it."""
    return _fidelity_qst("fidelity_qst", 4, state, target_state, conf_levels, n_measurements, n_trials, sampler, seed,
                         return_table, chunk)


def fidelity_qst_xl(state, target_state, conf_levels, n_measurements=1000, n_trials=100, *, sampler="numpy", seed=None,
                    return_table=False, chunk=None):
    """`fidelity_qst` up to five qubits: the same arguments and results, the same bits at n <= 4.  At n = 5 the
    programs (1023 variables) run on qt_lp_ineq_xl_batch, at most kLaunchProgramsXL of them per launch whatever
    `chunk` says; every (trial, level) costs two programs of 3.7 s (measured, profiles/lp_xl_timing.txt) on one compute
    unit each."""
    return _fidelity_qst("fidelity_qst_xl", 5, state, target_state, conf_levels, n_measurements, n_trials, sampler, seed,
                         return_table, chunk)


def _fidelity_qst(name, max_qubits, state, target_state, conf_levels, n_measurements, n_trials, sampler, seed, return_table,
                  chunk):
    n = state.n_qubits
    if n > max_qubits:
        raise NotImplementedError(f"{name} supports n <= {max_qubits} qubits (4^n - 1 <= {4**max_qubits - 1} LP variables); "
                                  f"got n = {n}")
    dim = 2**n
    probas, shots, weighted, A = qst_tables(state, n_measurements)
    c = np.asarray(target_state.bloch, dtype=np.float64)[1:]
    return _study(probas, shots, A, weighted[:, 0], c, float(dim), 1 / dim, True, conf_levels, n_trials, sampler, seed,
                  return_table, chunk)


def fidelity_qpt(channel, target_channel, conf_levels, n_measurements=1000, n_trials=100, input_states="sic", *,
                 sampler="numpy", seed=None, return_table=False, chunk=None):
    """Fidelity bounds of `n_trials` simulated process tomographies of `channel` with `target_channel` at each
    confidence level (the study of Fig. 2a; reference polytopes/notebooks/Fidelity.ipynb): 1/dim + min c . x and
    1/dim - min(-c . x) over A x <= f + delta - tile(W[:, 0]), dim = 4^n, n <= 2.  Results and keywords: see
    fidelity_qst."""
    n = channel.n_qubits
    if n > 2:
        raise NotImplementedError(f"fidelity_qpt supports n <= 2 qubits (16^n - 4^n <= 255 LP variables); got n = {n}")
    dim = 4**n
    probas, shots, weighted, states_matrix = qpt_tables(channel, n_measurements, input_states)
    A = process_matrix(states_matrix, weighted, dim)
    c = np.asarray(target_channel.choi.bloch, dtype=np.float64).reshape(dim, dim)[:, 1:].ravel()
    return _study(probas, shots, A, np.tile(weighted[:, 0], len(states_matrix)), c, 1.0, 1 / dim, False, conf_levels,
                  n_trials, sampler, seed, return_table, chunk)
