"""Coverage studies of the confidence intervals (reference quantpy/metrics.py:8-147, 150-319).

`get_CL_list_state` / `get_CL_list_channel` run `n_iter` experiments, build an interval for each, read the confidence
level at which the truth leaves it (metrics.py:140-144) and return the sorted levels: a calibrated interval gives the
uniform distribution.  The reference states the study as a Python loop over trials (and calls tomograph methods it no
longer has); here the trials are one batch.

interval='boot' (states, Hilbert-Schmidt distance, method_boot 'lin' / 'mle') is the nested bootstrap: every trial t
resamples `n_points` times around ITS OWN point estimate.  The resamples are laid out resample-major, row
(r * n_iter + t) of a chunk = resample r of trial t, which is the order `qt_device_multinomial` writes with
period = n_iter * S and the Born probabilities of the n_iter estimates as its table; one grouped launch family
(`qt_lin_dist_group_batch` / `qt_mle_dist_group_batch`: trial b against centre b % n_iter) reconstructs a chunk of whole
resamples and writes its distances, and `qt_group_hits` adds, per trial, how many of them lie below that trial's distance
to the truth.  Counts and distances never leave HBM; 8 * n_iter bytes come back.

`get_CL_list_state_boot(dst='hs' | 'trace' | 'if')` is that study in any of the three distances: for the trace distance and
the infidelity a chunk's estimates stay in a device workspace and `Engine.distance_dev` (`qt_metric_dist_dim`) measures
them.

interval='gamma' is `MomentInterval.radii_batch` over the batch of trials with the same rule.

`get_CL_list_state_mhmc` is the reference's interval='mhmc' branch for states: one Metropolis-Hastings chain per trial, all
of them in one launch that draws its own random numbers and returns, per trial, the hits and the accepted steps
(`qt_mhmc_state_hits`).  `get_CL_list_channel_mhmc` is the same branch for channels (n <= 2): a chain on the Choi vector
per trial with the CPTP projection in every step, `qt_mhmc_process_hits`.  Both take dst='hs' | 'trace' | 'if': for the
other two distances the chain kernels run the Jacobi-sweep metrics on the state they hold (`qt_mhmc_state_metric_hits`,
`qt_mhmc_process_metric_hits`).  `get_CL_list_channel_mhmc_large` is that study for channels of up to three qubits: at
n = 3 the chain is a launch family per step with the draws inside its kernels (`qt_mhmc_process_large_hits`,
`qt_mhmc_process_large_metric_hits`).  `get_CL_list_channel_boot_dst` is the process bootstrap study in any of the three: it
measures a chunk's Choi matrices the same way.  `get_CL_list_channel_boot_states` is that study with the resamples
reconstructed from their output states (method_boot='states'): a chunk's states by `lin_dev` / `mle_dev`, their Choi
matrices, the conditional CPTP projection and the distances by `qt_states_choi_dist_group_batch`.
"""
import numpy as np

from . import distributed as qdist
from .geometry import hs_dst, if_dst, trace_dst
from .sampling import SAMPLERS, device_chunks, shared_seed
from .tomography.interval import (_PROCESS_ERRORS, _STATE_ERRORS, BootstrapProcessInterval, MomentInterval, _agreed_flags,
                                  _distance_buffers, _error_flags, _raise_flagged)
from .tomography.process import ProcessTomograph
from .tomography.state import StateTomograph

_INTERVALS = ("gamma", "boot", "mhmc")
_CHUNK_BYTES = BootstrapProcessInterval._CHUNK_BYTES  # counts of one chunk of resamples
_PD_FLOOR = 1e-13  # get_CL_list_state_mhmc: an estimate starts a chain when estimate - _PD_FLOOR * 1 has a Cholesky factor


def levels_from_hits(hits, n_points):
    """metrics.py:140-144 on a sorted raw sample of `n_points` distances with CLs = np.linspace(0, 1, n_points): with
    hits = #{ i : delta > distances[i] } (the sample is sorted and a NaN, sorted last, is never below delta, so the last
    such index is hits - 1) the level is CLs[hits - 1], and 0 when nothing lies below delta."""
    hits = np.asarray(hits, dtype=np.int64)
    cls = np.linspace(0, 1, n_points)
    return np.where(hits > 0, cls[np.maximum(hits, 1) - 1], 0.0)


def _levels_from_radii(delta, radii, cls):
    """The same rule on tabulated radii (n_iter, n_points): CLs[last index with delta > radius], else 0."""
    below = delta[:, None] > radii
    last = below.shape[1] - 1 - np.argmax(below[:, ::-1], axis=1)
    return np.where(below.any(axis=1), cls[last], 0.0), below.sum(axis=1)


def _check_arguments(interval, dst, n_iter, n_points, sampler, boot_methods, method_boot):
    if interval not in _INTERVALS:
        raise ValueError("Incorrect value for argument `interval`.")
    if interval == "mhmc":
        raise NotImplementedError("interval='mhmc' (a chain per trial) is not implemented here; supported: 'gamma'"
                                  + (", 'boot'" if boot_methods else "")
                                  + ("; the chain study of a state is get_CL_list_state_mhmc" if boot_methods else
                                     "; the chain study of a channel is get_CL_list_channel_mhmc"))
    if interval == "boot" and not boot_methods:
        raise NotImplementedError("interval='boot' is not implemented by get_CL_list_channel (supported: 'gamma'); the "
                                  "bootstrap study of a channel is get_CL_list_channel_boot")
    if not (dst == "hs" or dst is hs_dst):
        raise NotImplementedError("only the Hilbert-Schmidt distance (dst='hs') is supported"
                                  + ("; the bootstrap study of a state in the trace distance or the infidelity is "
                                     "get_CL_list_state_boot" if boot_methods else ""))
    if interval == "boot" and method_boot not in boot_methods:
        raise NotImplementedError(f"interval='boot' supports method_boot in {boot_methods}, not {method_boot!r}")
    if int(n_iter) < 1 or int(n_points) < 1:
        raise ValueError("n_iter and n_points must be positive")
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, not {sampler!r}")


def _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, keyed):
    """(counts of the n_iter experiments, the resolved seed), the same on every rank: rank 0's stream (sampler='numpy',
    np.random's in the reference's order; the seed is resolved behind the draws, and only when `keyed` resamples will
    need it) or rank 0's Philox key (sampler='device')."""
    if sampler == "device":
        key = shared_seed(seed)
        return tmg.experiment_batch(n_measurements, povm, repeats=n_iter, sampler="device", seed=key), key
    counts = tmg.experiment_batch(n_measurements, povm, repeats=n_iter)
    if qdist.world()[1] > 1:
        counts = qdist.broadcast_array(counts)
    return counts, (shared_seed(seed) if keyed else None)


def _state_trials(state, n_iter, n_measurements, povm, sampler, seed, keyed, method, init, max_iter, tol):
    """The trials of a state study -> (tomograph, its engine, counts, resolved seed, estimates); an MLE that could not start
    raises LinAlgError."""
    tmg = StateTomograph(state, "hs")
    counts, base = _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, keyed)
    rho, info = tmg.point_estimate_batch(counts, method=method, init=init, max_iter=max_iter, tol=tol)
    if info is not None and np.any(info["status"] == 1):
        raise np.linalg.LinAlgError("starting point of the MLE is not positive definite")
    return tmg, tmg._engine(), counts, base, rho


def _chain_arguments(n_iter, n_points, burn_steps, thinning, sampler, dst):
    """The argument checks of the two chain studies -> (n_iter, n_points, burn_steps, thinning) as ints and the engine's
    name of `dst` (None: Hilbert-Schmidt)."""
    _check_arguments("gamma", "hs", n_iter, n_points, sampler, (), None)
    n_iter, n_points, burn_steps, thinning = int(n_iter), int(n_points), int(burn_steps), int(thinning)
    if thinning < 1:
        raise ValueError("thinning must be a positive integer")
    if burn_steps < 0:
        raise ValueError("burn_steps must not be negative")
    if burn_steps + n_points * thinning >= 2**32 - 1:
        raise ValueError("burn_steps + n_points * thinning must be below 2^32 - 1")
    metric = _distance_name(dst)
    return n_iter, n_points, burn_steps, thinning, None if metric == "hs" else metric


def _sharded_chain_hits(chain_hits, per_trial, *args, **kwargs):
    """(hits, accepted) of all trials: this rank's `shard_bounds` of the chains in one `chain_hits` launch on those rows
    of the `per_trial` arrays, chain = trial index, summed over the ranks."""
    n_iter = per_trial[0].shape[0]
    lo, hi = qdist.shard_bounds(n_iter)
    both = np.zeros((2, n_iter), dtype=np.int64)
    if hi > lo:
        both[0, lo:hi], both[1, lo:hi] = chain_hits(*(a[lo:hi] for a in per_trial), *args, first_chain=lo, **kwargs)
    if qdist.world()[1] > 1:
        both = qdist.allgather_equal(both).sum(0)
    return both


def _chunk_measure(eng, metric, shape, fused, reconstruct):
    """`measure(counts, centres, dist, status)` of `_chunked_hits`.  metric None: `fused`, the launch family that forms the
    Hilbert-Schmidt distances itself.  'trace' / 'if': `reconstruct(counts, mats, status)` into one workspace of `shape`
    matrices, allocated at the first chunk's size (a chunk starts at a whole resample, so its first row meets centre 0),
    and `Engine.distance_dev` on it."""
    if metric is None:
        return fused
    work = []

    def measure(counts, centres, dist, status):
        if not work:
            import torch

            work.append(torch.empty((counts.shape[0],) + shape, dtype=torch.complex128, device=counts.device))
        mats = work[0][:counts.shape[0]]
        reconstruct(counts, mats, status)
        eng.distance_dev(mats, centres, dist, metric)

    return measure


def _result(levels, return_details, **details):
    if return_details:
        return dict(levels=levels, **details)
    return np.sort(levels)


def get_CL_list_state(state, n_iter=1000, n_points=1000, interval="gamma", n_measurements=1000, method="lin",
                      method_boot="lin", dst="hs", povm="proj-set", physical=True, init="lin", tol=1e-3, max_iter=100,
                      step=0.01, burn_steps=1000, thinning=1, verbose=True, *, sampler="device", seed=None, chunk=None,
                      return_details=False):
    """Conducts `n_iter` experiments, constructs a confidence interval for each, computes the confidence level that
    corresponds to the distance between the target state and the point estimate, and returns the sorted levels
    (reference metrics.py:8-147; parameters as there).

    interval : 'gamma' -- `MomentInterval.radii_batch` at np.linspace(0, 1, n_points);
               'boot'  -- bootstrap around each trial's point estimate, `n_points` resamples reconstructed with
               `method_boot` in ('lin', 'mle') (`physical`, `init`, `tol`, `max_iter` as in BootstrapStateInterval), for
               dst='hs'.  'mhmc', other distances and other `method_boot` raise NotImplementedError.
    verbose is accepted and ignored: there is no loop to show.

    Keyword-only extensions
    sampler : 'device' (default) | 'numpy' -- how the TRIAL counts are drawn: on the GPU from Philox streams keyed by
        `seed`, or on np.random's global stream in the reference's order (`seed` then only keys the resamples).
    seed : 64-bit key; None takes one from np.random's stream (after the trial counts, with sampler='numpy').
    chunk : resamples per launch family of 'boot' (default: as many whole resamples as 256 MB of counts hold).
    return_details : return a dict of per-trial `counts`, `estimates`, `delta`, `hits`, `levels` in TRIAL order and
        `seed`, the key of the resamples, instead of the sorted levels.

    The resamples of 'boot' always come from the device sampler: trial t's probabilities depend on its estimate, so the
    nested loop has no reference stream to reproduce.  Keying: Philox key (resolve_seed(seed) + 1) mod 2^64, and row
    (r * n_iter + t) * S + s for setting s of resample r of trial t (S settings) -- a multinomial(n_measurements[s],
    clip(born_probs(estimate_t), 0, 1)[s]).  The table therefore depends neither on `chunk` nor on the number of ranks;
    with several ranks each takes `shard_bounds(n_points)` of the resamples, the hits are summed, and every rank returns
    the same list.  The level of trial t is np.linspace(0, 1, n_points)[hits_t - 1] (0 when hits_t == 0), hits_t the
    number of resampled distances strictly below delta_t (`levels_from_hits`)."""
    _check_arguments(interval, dst, n_iter, n_points, sampler, ("lin", "mle"), method_boot)
    n_iter, n_points = int(n_iter), int(n_points)
    tmg, eng, counts, base, rho = _state_trials(state, n_iter, n_measurements, povm, sampler, seed, interval == "boot",
                                                method, init, max_iter, tol)
    delta = eng.distance(rho, state.matrix)
    if interval == "gamma":
        cls = np.linspace(0, 1, n_points)
        levels, hits = _levels_from_radii(delta, MomentInterval(tmg).radii_batch(counts, cls), cls)
        return _result(levels, return_details, counts=counts, estimates=rho, delta=delta, hits=hits, seed=None)
    key = (base + 1) & (2**64 - 1)
    hits = _boot_hits(eng, tmg, rho, delta, n_points, key, method_boot, physical, init, tol, max_iter, chunk)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=rho, delta=delta, hits=hits,
                   seed=key)


def _distance_name(dst):
    for name, fn in (("hs", hs_dst), ("trace", trace_dst), ("if", if_dst)):
        if dst == name or dst is fn:
            return name
    raise ValueError("Invalid value for argument `dst` (supported: 'hs', 'trace', 'if')")


def get_CL_list_state_boot(state, n_iter=1000, n_points=1000, n_measurements=1000, method="lin", method_boot="lin", dst="hs",
                           povm="proj-set", physical=True, init="lin", tol=1e-3, max_iter=100, *, sampler="device",
                           seed=None, chunk=None, return_details=False):
    """The bootstrap study of a state -- `get_CL_list_state(interval='boot')`, parameters, keying of the resamples and
    details as there -- in any of the three distances: dst = 'hs' | 'trace' | 'if' (or the functions of
    quantpy_amd.geometry).  `delta` and the resampled distances are both measured in `dst`, as the reference's loop
    measures them (metrics.py:125-144 with the tomograph's dst).  (`get_CL_list_state` keeps its refusal of the other
    two; this is the study's name.)

    dst='hs' IS `get_CL_list_state(interval='boot')`: the same call, the same bits.  With 'trace' / 'if' the
    chunk's grouped reconstruction writes its density matrices into a device workspace (`Engine.lin_dev` / `mle_dev`),
    `Engine.distance_dev` measures resample r of trial t against estimate t (the table of the n_iter estimates, trial b
    against centre b % n_iter), and `group_hits` counts as before: counts, matrices and distances stay in HBM.  The
    distances are those of Hermitian arguments by the engine's Jacobi sweeps (include/qtomo.h: qt_metric_dist_dim), within
    1e-7 (trace) / 1e-6 (infidelity) of `trace_dst` / `if_dst` on the host."""
    metric = _distance_name(dst)
    if metric == "hs":
        return get_CL_list_state(state, n_iter, n_points, "boot", n_measurements, method, method_boot, "hs", povm, physical,
                                 init, tol, max_iter, sampler=sampler, seed=seed, chunk=chunk, return_details=return_details)
    _check_arguments("boot", "hs", n_iter, n_points, sampler, ("lin", "mle"), method_boot)
    n_iter, n_points = int(n_iter), int(n_points)
    tmg, eng, counts, base, rho = _state_trials(state, n_iter, n_measurements, povm, sampler, seed, True, method, init,
                                                max_iter, tol)
    delta = eng.distance(rho, state.matrix, metric)
    key = (base + 1) & (2**64 - 1)
    hits = _boot_hits(eng, tmg, rho, delta, n_points, key, method_boot, physical, init, tol, max_iter, chunk, metric)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=rho, delta=delta, hits=hits,
                   seed=key)


def get_CL_list_state_mhmc(state, n_iter=1000, n_points=1000, n_measurements=1000, method="lin", povm="proj-set", init="lin",
                           tol=1e-3, max_iter=100, step=0.01, burn_steps=1000, thinning=1, *, sampler="device", seed=None,
                           return_details=False, dst="hs"):
    """The interval='mhmc' branch of the reference's get_CL_list_state (metrics.py:125-144; parameters as
    there): `n_iter` experiments, for each a Metropolis-Hastings chain of the likelihood on the Cholesky parameters around
    ITS OWN point estimate (MHMCStateInterval: `burn_steps` steps, then n_points * thinning of which every `thinning`-th
    state is a sample), and the level at which the true state leaves the interval of the sampled distances.  Returns the
    sorted levels.  (`get_CL_list_state(interval='mhmc')` keeps its refusal; this is the study's name.)

    All chains of this rank's `shard_bounds(n_iter)` run in ONE launch (`Engine.mhmc_state_hits`): the proposal increments
    and uniforms are drawn on the device, the distance of every sample to the trial's estimate is formed where the state
    is held and compared with delta_t = hs_dst(estimate_t, state); per trial, the number of hits and of accepted steps come
    back.  Keying: Philox key (resolve_seed(seed) + 1) mod 2^64, chain = trial index t, step = burn-in first, then the
    sampling steps (include/qtomo.h: qt_mhmc_draws) -- the numbers of a trial depend neither on the number of ranks nor on
    its place in a batch, and never on np.random: the reference's stream is not reproduced.  The level of trial t is
    `levels_from_hits(hits_t, n_points)`.

    The chain starts at the Cholesky factor of the estimate, so an estimate that is not positive definite raises
    np.linalg.LinAlgError (on every rank), where the reference fails in scipy.linalg.cholesky.  The study is stricter than
    that call and than MHMCStateInterval, which start a chain wherever the factorisation goes through (`chol_param` status
    0): it asks for a factor of estimate - `_PD_FLOOR` * 1 (one more `chol_param` of the batch), that is, for a smallest
    eigenvalue above 1e-13.  The clipped 'lin' estimates of a rank-deficient state (a pure state, say) are such trials:
    the clip leaves them eigenvalues of 1e-15, which a factorisation in double precision takes or refuses by the sign of
    a rounding error.  (1e-13 is the size below which `qt_chol_param` stops trusting a pivot: a hundred times the clip,
    and far below the eigenvalues of an estimate of a full-rank state.)  Use a mixed state, or method='mle' on one.

    dst (keyword-only) = 'hs' | 'trace' | 'if', or the functions of quantpy_amd.geometry: the distance of the study.  'hs'
    is the call described above, the same bits.  Otherwise delta_t = `Engine.distance`(estimate_t, state, dst) and the
    chains run through `Engine.mhmc_state_hits(metric=dst)`: the same chains (the accepted steps do not depend on the
    distance) with every sample measured as `metric_dist` measures it, by the same device functions in the kernel that
    holds the sample (include/qtomo.h: qt_mhmc_state_metric_hits).

    Four- and five-qubit states run the same study through the same two methods (one workgroup per chain; include/qtomo.h:
    qt_mhmc_state_large_hits, qt_mhmc_state_large_metric_hits); arguments, keying, sharding and details are those above.
    At the default 1000 shots per setting the 'lin' estimates of a four- or five-qubit state are not positive definite
    even for a state as mixed as GHZ / 2 + 1 / 2d (smallest eigenvalue of the unclipped estimate about -0.003 at n = 4
    and -0.02 at n = 5, against +0.020 at 10 000 and +0.012 at 100 000 shots), so the study raises LinAlgError there, as
    stated above.  The remedy: more shots (`n_measurements`), or method='mle'.

    `sampler`, `seed`, `return_details` as in `get_CL_list_state`; the details also hold `acceptance_rate`, per trial the
    accepted post-burn steps / (n_points * thinning), the reference's definition."""
    n_iter, n_points, burn_steps, thinning, metric = _chain_arguments(n_iter, n_points, burn_steps, thinning, sampler, dst)
    tmg, eng, counts, base, rho = _state_trials(state, n_iter, n_measurements, povm, sampler, seed, True, method, init,
                                                max_iter, tol)
    delta = eng.distance(rho, state.matrix, metric)
    x0, status = eng.chol_param(rho)
    # ... and none for the estimate less the floor: its smallest eigenvalue is not above _PD_FLOOR (a NaN is refused too)
    _, shifted = eng.chol_param(rho - _PD_FLOOR * np.eye(rho.shape[-1]))
    bad = (status != 0) | (shifted != 0)
    if np.any(bad):  # (the same estimates on every rank: all raise, or none)
        raise np.linalg.LinAlgError(f"the estimate of trial {int(np.flatnonzero(bad)[0])} is not positive definite: "
                                    "no Cholesky factor to start its chain from")
    key = (base + 1) & (2**64 - 1)
    hits, accepted = _sharded_chain_hits(eng.mhmc_state_hits, (counts, rho, x0, delta), key, burn_steps, n_points, thinning,
                                         step, metric=metric)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=rho, delta=delta, hits=hits,
                   seed=key, acceptance_rate=accepted / (n_points * thinning))


def _boot_hits(eng, tmg, rho, delta, n_points, key, method_boot, physical, init, tol, max_iter, chunk, metric=None):
    """hits[t] = #{ r < n_points : delta_t > hs_dst(estimate(resample r of trial t), estimate_t) }, this rank's shard of
    the resamples chunk by chunk on the device, summed over the ranks.  `metric` = 'trace' / 'if': that distance in the
    place of hs_dst, formed from the chunk's density matrices (`_chunk_measure`)."""
    n_iter = rho.shape[0]
    pvals = np.clip(eng.born_probs(eng.bloch_from_matrix(rho)), 0, 1).reshape(n_iter * eng.S, eng.K)
    if method_boot == "lin":
        opts = dict(physical=physical)
        fused, plain = eng.lin_dist_dev, eng.lin_dev
    else:
        opts = dict(init=init, max_iter=max_iter, tol=tol)
        fused, plain = eng.mle_dist_dev, eng.mle_dev
    measure = _chunk_measure(eng, metric, (eng.d, eng.d),
                             lambda counts, centres, dist, status: fused(counts, centres, dist, status=status, **opts),
                             lambda counts, mats, status: plain(counts, mats, status=status, **opts))
    return _chunked_hits(eng, rho, (eng.S, eng.K), pvals, tmg.n_measurements, delta, n_points, key, chunk, measure,
                         _STATE_ERRORS)


def _chunked_hits(eng, centres, trial_shape, pvals, shots, delta, n_points, key, chunk, measure, errors):
    """The chunk loop of both nested bootstraps.  `centres` (n_iter, ., .) are the trials' estimates, one trial's counts
    have shape `trial_shape` = (..., S, K), `pvals` is the table of the n_iter estimates (rows of K) and `shots` the (S,)
    totals of a setting.  This rank's `shard_bounds(n_points)` of the resamples runs in chunks of whole resamples
    (`sampling.device_chunks`: a resample of all trials is the unit of the table keyed by `key`) through
    `measure(counts, centres, dist, status)` -- a grouped launch family on device tensors -- and `group_hits` against
    `delta`.  The `errors` seen in a chunk (interval._error_flags), OR-ed over chunks and ranks (one all-gather, then
    the one of the hits), are raised in order: every rank raises, or none.  Returns hits (n_iter,) summed over the ranks."""
    import torch

    n_iter = centres.shape[0]
    n_out = trial_shape[-1]
    rows = int(np.prod(trial_shape[:-1])) * n_iter  # table rows per resample of all trials
    shots = np.atleast_1d(np.asarray(shots))
    per_resample = rows * n_out * 8
    chunk = int(chunk) if chunk else max(1, _CHUNK_BYTES // per_resample)
    # The batch size of a launch is a 32-bit int.  (A caller's `chunk` is otherwise taken as given: the count buffer
    # is chunk * per_resample bytes, and only the default is held to _CHUNK_BYTES.)
    chunk = max(1, min(chunk, (2**31 - 1) // n_iter))
    lo, hi = qdist.shard_bounds(n_points)
    chunk = min(chunk, max(hi - lo, 1))
    dist, status, centres = _distance_buffers(eng, chunk * n_iter, centres)
    thr = torch.from_numpy(np.ascontiguousarray(delta, dtype=np.float64)).to(dist.device)
    hits = torch.zeros(n_iter, dtype=torch.int64, device=dist.device)
    bad = None
    for _, counts in device_chunks(eng, np.tile(shots, rows // len(shots)), np.reshape(pvals, (rows, n_out)), rows, lo, hi,
                                   chunk, key, (n_iter,) + tuple(trial_shape)):
        counts = counts.flatten(0, 1)  # row r * n_iter + t = resample r of trial t
        b = counts.shape[0]
        measure(counts, centres, dist[:b], status[:b])
        eng.group_hits(dist[:b], thr, hits)
        seen = _error_flags(status[:b], errors)
        bad = seen if bad is None else bad | seen
    eng.sync()
    bad = _agreed_flags(_error_flags(status[:0], errors) if bad is None else bad)  # (None: a rank without resamples)
    hits = hits.cpu().numpy()
    if qdist.world()[1] > 1:
        hits = qdist.allgather_equal(hits).sum(0)
    _raise_flagged(bad, errors)
    return hits


def get_CL_list_channel(channel, n_iter=1000, interval="gamma", n_points=1000, n_measurements=1000, method="lifp",
                        method_boot="lifp", dst="hs", povm="proj-set", input_states="proj4", cptp=True, tol=1e-3,
                        states_physical=True, states_init="lin", states_est_method="lin", states_est_method_boot="lin",
                        step=0.01, burn_steps=1000, thinning=1, verbose=True, *, sampler="device", seed=None,
                        return_details=False):
    """The same study for a channel and its Choi matrix (reference metrics.py:150-319; parameters as there), for
    interval='gamma': the process form of `MomentInterval.radii_batch` at np.linspace(0, 1, n_points).  'boot' and
    'mhmc' raise NotImplementedError; the bootstrap study of a channel is `get_CL_list_channel_boot` (method_boot='lifp')
    or `get_CL_list_channel_boot_states` (method_boot='states'), the chain study `get_CL_list_channel_mhmc`.  `sampler`,
    `seed`, `return_details` as in `get_CL_list_state`."""
    _check_arguments(interval, dst, n_iter, n_points, sampler, (), method_boot)
    n_iter, n_points = int(n_iter), int(n_points)
    tmg = ProcessTomograph(channel, input_states, "hs")
    counts, _ = _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, False)
    choi = tmg.point_estimate_batch(counts, method=method, states_est_method=states_est_method, states_init=states_init)
    delta = tmg._engine().distance(choi, channel.choi.matrix)
    cls = np.linspace(0, 1, n_points)
    levels, hits = _levels_from_radii(delta, MomentInterval(tmg).radii_batch(counts, cls), cls)
    return _result(levels, return_details, counts=counts, estimates=choi, delta=delta, hits=hits, seed=None)


def get_CL_list_channel_boot(channel, n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                             input_states="proj4", cptp=True, states_init="lin", states_est_method="lin", *,
                             sampler="device", seed=None, chunk=None, return_details=False):
    """The interval='boot', method_boot='lifp', dst='hs' branch of the reference's get_CL_list_channel
    (metrics.py:282-316; parameters as there): `n_iter` process tomographies, each bootstrapped with `n_points` resamples
    around ITS OWN Choi estimate; the level of trial t is the one at which the true Choi matrix leaves its interval.
    Returns the sorted levels.  (`get_CL_list_channel(interval='boot')` keeps its refusal; this is the study's name.)

    The trials are formed as in `get_CL_list_channel`: `point_estimate_batch(counts, method=method, ...)` with its default
    cptp=True, as the reference's loop calls it; `cptp` is what the RESAMPLES are reconstructed with ('lifp', `tol` not
    passed: BootstrapProcessInterval's loop).  `sampler`, `seed`, `chunk`, `return_details` as in `get_CL_list_state`.

    Keying of the resamples (always the device sampler): Philox key (resolve_seed(seed) + 1) mod 2^64, and row
    ((r * n_iter + t) * D + i) * S + s for setting s of input state i of resample r of trial t (D = 4^n input states, S
    settings) -- a multinomial(n_measurements[s], `Engine.process_born_probs`(estimates)[t, i, s]).  The table depends
    neither on `chunk` nor on the number of ranks; each rank takes `shard_bounds(n_points)` of the resamples, the hits are
    summed and every rank returns the same list.  A chunk of whole resamples is one `device_multinomial`, one
    `qt_lifp_dist_group_batch` (process b against centre b % n_iter) and one `qt_group_hits`; the level of trial t is
    `levels_from_hits`: np.linspace(0, 1, n_points)[hits_t - 1], hits_t the resampled distances strictly below delta_t.

    The same study in the trace distance or the infidelity is `get_CL_list_channel_boot_dst`."""
    return _channel_boot(channel, n_iter, n_points, n_measurements, method, povm, input_states, cptp, states_init,
                         states_est_method, sampler, seed, chunk, return_details, "hs")


def get_CL_list_channel_boot_dst(channel, n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                                 input_states="proj4", cptp=True, states_init="lin", states_est_method="lin", *,
                                 sampler="device", seed=None, chunk=None, return_details=False, dst="hs"):
    """`get_CL_list_channel_boot` -- parameters, keying of the resamples and details as there -- in any of the three
    distances: dst = 'hs' | 'trace' | 'if', or the functions of quantpy_amd.geometry, as `get_CL_list_state_boot` is for
    states.  (`get_CL_list_channel_boot` keeps the argument list its callers and tests know; this is the study's name
    with a distance.)

    dst='hs' IS `get_CL_list_channel_boot`: the same call, the same bits.  Otherwise `delta` and the resampled distances
    are measured in `dst`: a chunk's Choi matrices go into one device workspace of the first chunk's size
    (`Engine.lifp_dev`) and `Engine.distance_dev` measures resample r of trial t against estimate t (the table of
    the n_iter estimates, process b against centre b % n_iter), as `_boot_hits` does it for states; n <= 3 (dim = 4, 16, 64).
    A Choi matrix here has trace 2^n, not 1, so `if_dst` of two of them is 1 - (about 2^n)^2 < 1e-15 and comes back as 0,
    exactly as geometry.py:52-54 returns it in the reference.  dst='if' on a channel is therefore accepted and faithful,
    and degenerate: every distance, every `delta` and every level is 0."""
    return _channel_boot(channel, n_iter, n_points, n_measurements, method, povm, input_states, cptp, states_init,
                         states_est_method, sampler, seed, chunk, return_details, dst)


def _channel_boot(channel, n_iter, n_points, n_measurements, method, povm, input_states, cptp, states_init,
                  states_est_method, sampler, seed, chunk, return_details, dst):
    _check_arguments("boot", "hs", n_iter, n_points, sampler, ("lifp",), "lifp")
    metric = _distance_name(dst)
    metric = None if metric == "hs" else metric
    n_iter, n_points = int(n_iter), int(n_points)
    tmg = ProcessTomograph(channel, input_states, "hs")
    counts, base = _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, True)
    choi = tmg.point_estimate_batch(counts, method=method, states_est_method=states_est_method, states_init=states_init)
    eng = tmg._engine()
    delta = eng.distance(choi, channel.choi.matrix, metric)
    key = (base + 1) & (2**64 - 1)
    pvals = eng.process_born_probs(choi)
    measure = _chunk_measure(eng, metric, (eng.D, eng.D),
                             lambda counts, centres, dist, status: eng.lifp_dist_dev(counts, centres, dist, cptp=cptp,
                                                                                     status=status),
                             lambda counts, mats, status: eng.lifp_dev(counts, mats, cptp=cptp, status=status))
    hits = _chunked_hits(eng, choi, (eng.D, eng.S, eng.K), pvals, tmg.tomographs[0].n_measurements, delta, n_points,
                         key, chunk, measure, _PROCESS_ERRORS)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=choi, delta=delta, hits=hits,
                   seed=key)


# What a chunk of 'states' resamples raises, in order (the codes are those `_states_boot_measure` writes per process).
_STATES_BOOT_ERRORS = ((1, np.linalg.LinAlgError, "starting point of the MLE is not positive definite"),
                       (2, ValueError, _PROCESS_ERRORS[0][2]))


def get_CL_list_channel_boot_states(channel, n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                                    input_states="proj4", cptp=True, states_physical=True, states_init="lin",
                                    states_est_method="lin", states_est_method_boot="lin", *, sampler="device", seed=None,
                                    chunk=None, return_details=False, dst="hs"):
    """The interval='boot', method_boot='states' branch of the reference's get_CL_list_channel (metrics.py:299-309;
    parameters as there): `n_iter` process tomographies, each bootstrapped with `n_points` resamples around ITS OWN Choi
    estimate, every resample reconstructed from its output states.  Returns the sorted levels.
    (`get_CL_list_channel(interval='boot')` keeps its refusal; this is the study's name.)

    Trials, `delta`, the Philox keying of the resamples, sharding over the ranks, chunking by whole resamples, `sampler`,
    `seed`, `chunk`, `return_details` and `dst` = 'hs' | 'trace' | 'if' are exactly those of `get_CL_list_channel_boot_dst`.
    A resample is reconstructed as `point_estimate_batch(counts, method='states', cptp=cptp,
    states_est_method=states_est_method_boot, states_physical=states_physical, states_init=states_init)` reconstructs it,
    that method's other defaults included (an 'mle' of at most 1000 iterations with tol 1e-10).  states_est_method_boot
    outside ('lin', 'mle') raises NotImplementedError before any device work.

    A chunk never leaves the device: `device_multinomial`; `Engine.lin_dev` / `mle_dev` on its chunk * n_iter * D count
    tensors into one workspace of the first chunk's size; `Engine.states_choi_dist_dev` against the table of the n_iter
    estimates (process b against centre b % n_iter) for 'hs', or `states_choi_dev` and `distance_dev` for 'trace' / 'if';
    `group_hits`.  (With cptp the number of resamples that fail the CPTP test comes back to the host, once per slice of
    `qt_states_choi_batch`: it sizes the projection's launch.)  An output-state MLE that cannot start raises
    np.linalg.LinAlgError, a resample without a finite Choi matrix ValueError, on every rank."""
    if states_est_method_boot not in ("lin", "mle"):
        raise NotImplementedError("get_CL_list_channel_boot_states supports states_est_method_boot in ('lin', 'mle'), not "
                                  f"{states_est_method_boot!r}")
    _check_arguments("boot", "hs", n_iter, n_points, sampler, ("lifp",), "lifp")
    metric = _distance_name(dst)
    metric = None if metric == "hs" else metric
    n_iter, n_points = int(n_iter), int(n_points)
    tmg = ProcessTomograph(channel, input_states, "hs")
    counts, base = _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, True)
    choi = tmg.point_estimate_batch(counts, method=method, states_est_method=states_est_method, states_init=states_init)
    eng = tmg._engine()
    delta = eng.distance(choi, channel.choi.matrix, metric)
    key = (base + 1) & (2**64 - 1)
    pvals = eng.process_born_probs(choi)
    measure = _states_boot_measure(eng, tmg._states_weights(), metric, states_est_method_boot, states_physical, states_init,
                                   cptp)
    hits = _chunked_hits(eng, choi, (eng.D, eng.S, eng.K), pvals, tmg.tomographs[0].n_measurements, delta, n_points,
                         key, chunk, measure, _STATES_BOOT_ERRORS)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=choi, delta=delta, hits=hits,
                   seed=key)


def _states_boot_measure(eng, weights, metric, method_boot, physical, init, cptp):
    """`measure(counts, centres, dist, status)` of `_chunked_hits` for the 'states' resamples: the chunk's b * D output
    states by `lin_dev` / `mle_dev` (the MLE with point_estimate_batch's defaults n_iter = 1000, tol = 1e-10) into one
    workspace of the first chunk's size, then the Choi matrices and their distances.  status[p] of process p: 1 where an
    output-state MLE could not start, else 2 where an output state is not finite, else 0."""
    work = {}

    def measure(counts, centres, dist, status):
        import torch

        b, dd = counts.shape[0], eng.D
        if not work:
            dev = counts.device
            work["states"] = torch.empty((b * dd, eng.d, eng.d), dtype=torch.complex128, device=dev)
            work["status"] = torch.zeros(b * dd, dtype=torch.int32, device=dev)
            work["weights"] = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.complex128)).to(dev)
            if metric is not None:
                work["choi"] = torch.empty((b, dd, dd), dtype=torch.complex128, device=dev)
        states, state_status = work["states"][:b * dd], work["status"][:b * dd]
        flat = counts.reshape(b * dd, eng.S, eng.K)
        if method_boot == "lin":
            eng.lin_dev(flat, states, physical=physical, status=state_status)
        else:
            eng.mle_dev(flat, states, init=init, max_iter=1000, tol=1e-10, status=state_status)
        per_process = states.view(b, dd, eng.d, eng.d)
        if metric is None:
            eng.states_choi_dist_dev(per_process, work["weights"], centres, dist, cptp=cptp)
        else:
            choi = work["choi"][:b]
            eng.states_choi_dev(per_process, work["weights"], choi, cptp=cptp)
            eng.distance_dev(choi, centres, dist, metric)
        no_start = (state_status.view(b, dd) == 1).any(dim=1)
        finite = torch.isfinite(torch.view_as_real(states).view(b, -1)).all(dim=1)
        status.copy_(torch.where(no_start, 1, torch.where(finite, 0, 2)).to(torch.int32))

    return measure


def get_CL_list_channel_mhmc(channel, n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                             input_states="proj4", states_init="lin", states_est_method="lin", step=0.01, burn_steps=1000,
                             thinning=1, *, sampler="device", seed=None, return_details=False, dst="hs"):
    """The interval='mhmc' branch of the reference's get_CL_list_channel (metrics.py:289-298; parameters as
    there): `n_iter` process tomographies, for each a Metropolis-Hastings chain of the likelihood on the Choi vector around
    ITS OWN estimate (MHMCProcessInterval with use_new_estimate=False: every proposal projected onto the CPTP set,
    `burn_steps` steps, then n_points * thinning of which every `thinning`-th state is a sample, the samples' real parts
    measured against the estimate), and the level at which the true Choi matrix leaves the interval of the sampled
    distances.  Returns the sorted levels.  (`get_CL_list_channel(interval='mhmc')` keeps its refusal; this is the study's
    name.)  One and two qubits: a channel of more qubits raises NotImplementedError; `get_CL_list_channel_mhmc_large` is
    the same study for one to three qubits.

    The trials are formed as in `get_CL_list_channel_boot` (`point_estimate_batch` with its default cptp=True).  All
    chains of this rank's `shard_bounds(n_iter)` run in ONE launch (`Engine.mhmc_process_hits`), chain t from its own
    estimate, which is also its centre: the proposal increments and uniforms are drawn on the device, the distance of
    every sample is formed where the state is held and compared with delta_t = hs_dst(estimate_t, Choi matrix of the
    channel); per trial, the number of hits and of accepted steps come back.  Keying: Philox key
    (resolve_seed(seed) + 1) mod 2^64, chain = trial index t, step = burn-in first, then the sampling steps
    (include/qtomo.h: qt_mhmc_process_draws) -- the numbers of a trial depend neither on the number of ranks nor on its
    place in a batch, and never on np.random.  The level of trial t is `levels_from_hits(hits_t, n_points)`.

    dst (keyword-only) = 'hs' | 'trace' | 'if', or the functions of quantpy_amd.geometry: 'hs' is the call described
    above, the same bits.  Otherwise delta_t = `Engine.distance`(estimate_t, Choi matrix of the channel, dst) and the
    chains run through `Engine.mhmc_process_hits(metric=dst)`: the same chains with the real part of every sample
    measured as `metric_dist` measures it, in the kernel that holds the sample (include/qtomo.h:
    qt_mhmc_process_metric_hits).
    A Choi matrix here has trace 2^n, not 1, so `if_dst` of two of them is 1 - (about 2^n)^2 < 1e-15 and comes back as 0,
    exactly as geometry.py:52-54 returns it in the reference.  dst='if' on a channel is therefore accepted and faithful,
    and degenerate: every distance, every `delta` and every level is 0.

    An estimate that is not finite (an input state without counts) raises ValueError on every rank.  `sampler`, `seed`,
    `return_details` as in `get_CL_list_state`; the details also hold `acceptance_rate`, per trial the accepted post-burn
    steps / (n_points * thinning), the reference's definition."""
    chain = _chain_arguments(n_iter, n_points, burn_steps, thinning, sampler, dst)
    if channel.n_qubits > 2:
        raise NotImplementedError(f"get_CL_list_channel_mhmc runs channels of one and two qubits, not {channel.n_qubits}: "
                                  "the chain of a three-qubit process has no fused kernel")
    return _channel_mhmc_study(channel, chain, n_measurements, method, povm, input_states, states_init, states_est_method,
                               step, sampler, seed, return_details)


def _channel_mhmc_study(channel, chain, n_measurements, method, povm, input_states, states_init, states_est_method, step,
                        sampler, seed, return_details):
    """The body of `get_CL_list_channel_mhmc` and `get_CL_list_channel_mhmc_large`; `chain`: what `_chain_arguments`
    returned.  `Engine.mhmc_process_hits` picks the library's entry by the size of the channel."""
    n_iter, n_points, burn_steps, thinning, metric = chain
    tmg = ProcessTomograph(channel, input_states, "hs")
    counts, base = _trial_counts(tmg, n_measurements, povm, n_iter, sampler, seed, True)
    choi = tmg.point_estimate_batch(counts, method=method, states_est_method=states_est_method, states_init=states_init)
    if not np.all(np.isfinite(choi)):  # (the same estimates on every rank: all raise, or none)
        raise ValueError("a trial has no finite Choi matrix (an input state without counts)")
    eng = tmg._engine()
    delta = eng.distance(choi, channel.choi.matrix, metric)
    key = (base + 1) & (2**64 - 1)
    hits, accepted = _sharded_chain_hits(eng.mhmc_process_hits, (counts, choi, choi, delta), key, burn_steps, n_points,
                                         thinning, step, metric=metric)
    return _result(levels_from_hits(hits, n_points), return_details, counts=counts, estimates=choi, delta=delta, hits=hits,
                   seed=key, acceptance_rate=accepted / (n_points * thinning))


def get_CL_list_channel_mhmc_large(channel, n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                                   input_states="proj4", states_init="lin", states_est_method="lin", step=0.01,
                                   burn_steps=1000, thinning=1, *, sampler="device", seed=None, return_details=False,
                                   dst="hs"):
    """`get_CL_list_channel_mhmc` for channels of one, two and three qubits: the same study, arguments, defaults, keying,
    sharding and details.  At n <= 2 it is that function -- the same bits; that name refuses three qubits, this one serves
    them.  A channel of more than three qubits raises NotImplementedError.

    n = 3: the chains run through `qt_mhmc_process_large_hits` / `qt_mhmc_process_large_metric_hits` (include/qtomo.h): per
    step the launches of `Engine.mhmc_process` at n = 3 -- proposal, CPTP projection, model and NLL, accept test -- with the
    numbers of `Engine.mhmc_draws_dim(4096, ...)` drawn inside the proposing and the deciding kernel, and the kept state
    measured where it lies; per trial the hits and the accepted steps come back.  The chains of a rank run in slices of
    1024 (QT_OPT_MHMC_PROCESS_SLICE), about 0.6 MB of workspace per chain of a slice.

    `step` must be chosen for the shots: the process likelihood uses the raw counts and sharpens with them.  At
    n_measurements = 10 000 per setting step = 1e-5 accepts about half of the proposals of a three-qubit chain
    (tests/test_gpu_batch_positions.py); the default step = 0.01 accepts nothing at n = 3.

    Cost at n = 3 (profiles/process_mhmc_large_coverage_timing.txt; depolarizing channel, 10 000 shots, step 1e-5): the
    defaults' 2000 steps of 1000 chains take 3.3 s end to end in 'hs' and 7.4 s in 'trace', 1.5 / 3.6 ms per step; the CPTP
    projection (1.0 ms) and the model and NLL (0.6 ms) make up an 'hs' step, the 64 x 64 eigen-solves (4.2 ms per kept
    step) most of a 'trace' one."""
    chain = _chain_arguments(n_iter, n_points, burn_steps, thinning, sampler, dst)
    if channel.n_qubits > 3:
        raise NotImplementedError(f"get_CL_list_channel_mhmc_large runs channels of one to three qubits, not "
                                  f"{channel.n_qubits}")
    return _channel_mhmc_study(channel, chain, n_measurements, method, povm, input_states, states_init, states_est_method,
                               step, sampler, seed, return_details)
