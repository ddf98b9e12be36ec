"""Bootstrap confidence intervals (reference quantpy/tomography/interval.py:19-56, 542-685).

The reference resamples in a serial Python loop: experiment -> point_estimate -> distance.  Here
the loop only draws the counts (host RNG, same call order, so a seed gives the same resamples);
all resamples are then reconstructed in one batched launch, sharded over the ranks of the
process group when there is one, and the distances are all-gathered (quantpy_amd.distributed).

`MomentInterval` (reference interval.py:59-110 with stats.py:21-47) is the closed-form interval the
reference's CLI scripts use: the first two moments of the squared Hilbert-Schmidt error of the
linear-inversion estimate under multinomial noise, matched to a gamma / normal / exponential
law.  Its one heavy step, the left inverse of the (state or process) design matrix, runs on the GPU
(qt_left_inverse), and so do the moment sums (qt_moment_batch: the reference's six-operand einsums collected into
O(M^2) matrix form, batched over trials).

`MHMCStateInterval` / `MHMCProcessInterval` run their chains on the GPU (qt_mhmc_state / qt_mhmc_process);
`SugiyamaInterval` and `HolderInterval` are closed-form / compositions over those.

The two state intervals the reference builds on cvxopt give fidelity bounds against a target state.
`PolytopeStateInterval` (Kiktenko et al., arXiv:2109.04734; reference interval.py:268-335) solves its 2 * n_points
linear programs, which share one constraint matrix, in ONE launch of the batched interior-point solver
(qt_lp_ineq_batch).  `MomentFidelityStateInterval` (interval.py:113-160) poses one second-order cone program per
confidence level whose optimum has a closed form (a linear objective over a ball cut by a hyperplane), so it needs no
solver.  Their process counterparts (MomentFidelityProcessInterval, PolytopeProcessInterval) are still names that
raise NotImplementedError.
"""
from abc import ABC, abstractmethod
from enum import Enum, auto

import numpy as np
from scipy.interpolate import interp1d

import scipy.stats as sts

from .. import _capi
from .. import distributed as qdist
from ..engine import get_engine
from ..geometry import hs_dst, if_dst, trace_dst
from ..routines import _left_inv
from ..sampling import check_pvals, device_chunks, shared_seed


class Mode(Enum):
    STATE = auto()
    CHANNEL = auto()


def _proposal_increments(dim):
    """size -> (size, dim) proposal increments of a chain, drawn as the reference draws them: scipy's frozen
    `multivariate_normal(mean=zeros(dim))` (mhmc.py / interval.py:735-738, :822-825) on np.random's global stream.
    That call ends in `RandomState.multivariate_normal`, which draws standard_normal((size, dim)) and multiplies by
    sqrt(s) v of svd(cov); for the identity covariance LAPACK returns s = 1, v = I exactly, so the product is the draws
    themselves.  Up to dim 256 the reference's own call is made; above (five-qubit states: dim 1024; three-qubit
    processes: dim 4096, where the eigen-decomposition in the constructor and the SVD per call cost ~20 s each) the
    draws are taken directly -- the n = 5 state chain of tests/golden/mhmc_large.npz and the n = 3 process chains of
    tests/golden/mhmc3.npz, made by the reference through the full call, pin the equivalence."""
    if dim <= 256:
        from scipy.stats import multivariate_normal

        frozen = multivariate_normal(mean=np.zeros(dim))
        return lambda size: frozen.rvs(size=size).reshape(size, dim)
    return lambda size: np.random.standard_normal((size, dim))


def _engine_metric(dst, n_qubits, max_qubits=5):
    """'trace' / 'if' when `dst` is the trace distance / infidelity and the engine forms it (Engine.distance), else None.
    `max_qubits`: the largest object the caller hands over -- 6 for the Choi matrix of a three-qubit channel (dim 64)."""
    if n_qubits > max_qubits:
        return None
    return "trace" if dst is trace_dst else "if" if dst is if_dst else None


def _levels_or_default(conf_levels):
    """The grid of confidence levels every interval is evaluated on when the caller names none."""
    return np.linspace(1e-3, 1 - 1e-3, 1000) if conf_levels is None else conf_levels


def _pop_hidden_keys(kwargs):
    return {k: v for k, v in kwargs.items() if k not in ("self", "tmg") and not k.startswith("__")}


class ConfidenceInterval(ABC):
    """Functor: `interval(conf_levels)` -> (distances, conf_levels)."""

    EPS = 1e-15

    def __init__(self, tmg, **kwargs):
        self.tmg = tmg
        if hasattr(tmg, "state"):
            self.mode = Mode.STATE
        elif hasattr(tmg, "channel"):
            self.mode = Mode.CHANNEL
        else:
            raise ValueError()
        for name, value in kwargs.items():
            setattr(self, name, value)

    def __call__(self, conf_levels=None):
        conf_levels = _levels_or_default(conf_levels)
        if not hasattr(self, "cl_to_dist"):
            self.setup()
        return self.cl_to_dist(conf_levels), conf_levels

    @abstractmethod
    def setup(self):
        """Build `self.cl_to_dist`."""

    def _finish(self, dist):
        dist = np.sort(dist)
        self.cl_to_dist = interp1d(np.linspace(0, 1, len(dist)), dist)


class MomentInterval(ConfidenceInterval):
    """Closed-form interval from the first two moments of the squared HS error of linear inversion.
    distr_type : 'gamma' (default) | 'norm' | 'exp'.

    Both heavy steps run on the GPU: the left inverse of the design matrix (qt_left_inverse: MFMA Gram, pivoted
    Gauss-Jordan) and the moment sums of stats.py:21-47 (qt_moment_batch; qt_moment_freq_batch when `results` are not
    integers, which the reference accepts; a three-qubit process, 13 824 POVM rows, included).  `radii_batch` evaluates the interval for
    a whole batch of count tensors of the same experiment in one launch -- the coverage study of
    notebooks/Verification.ipynb (10 000 trials per state) is that call."""

    def __init__(self, tmg, distr_type="gamma"):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    def _design(self):
        """(dim, n_measurements (S,), counts (S, K), inv_matrix (rows, S*K)) as interval.py:72-87 builds them."""
        tmg = self.tmg
        if self.mode == Mode.STATE:
            dim = 2**tmg.state.n_qubits
            n_measurements = tmg.n_measurements
            counts = np.asarray(tmg.results)
            povm = np.asarray(tmg.povm_matrix)
            design = povm.reshape(-1, povm.shape[-1])
        else:
            dim = 4**tmg.channel.n_qubits
            first = tmg.tomographs[0]
            n_measurements = np.tile(first.n_measurements, len(tmg.tomographs))
            counts = np.vstack([t.results for t in tmg.tomographs])
            povm = np.asarray(first.povm_matrix)
            povm_rows = povm.reshape(-1, povm.shape[-1])
            states = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements])
            design = np.einsum("sd,pi->spdi", states, povm_rows).reshape(states.shape[0] * povm_rows.shape[0], -1)
        inv_matrix = np.asarray(_left_inv(design)) / dim  # GPU: Gram GEMM (MFMA), pivoted Gauss-Jordan, GEMM
        return dim, np.asarray(n_measurements, dtype=np.float64), counts, inv_matrix

    def _engine(self):
        tmg = self.tmg
        return get_engine(tmg.state.n_qubits if self.mode == Mode.STATE else tmg.channel.n_qubits)

    def _distribution(self, mean, variance):
        if self.distr_type == "norm":
            return sts.norm(loc=mean, scale=np.sqrt(variance))
        if self.distr_type == "gamma":
            scale = variance / mean
            return sts.gamma(a=mean / scale, scale=scale)
        if self.distr_type == "exp":
            return sts.expon(scale=mean)
        raise NotImplementedError(f"Unsupported distribution type {self.distr_type}")

    def _alpha(self, dim):
        if self.tmg.dst == hs_dst:
            return np.sqrt(dim / 2)
        if self.tmg.dst == trace_dst:
            return dim / 2
        raise NotImplementedError()

    def setup(self):
        dim, n_measurements, counts, inv_matrix = self._design()
        mean, variance = self._engine().moments(counts, n_measurements, inv_matrix)
        distr = self._distribution(mean, variance)
        alpha = self._alpha(dim)
        self.mean, self.variance = mean, variance
        self.cl_to_dist = lambda cl: np.sqrt(distr.ppf(cl)) * alpha

    def radii_batch(self, counts, conf_levels):
        """The interval's radii for B count tensors of this tomograph's experiment (same POVM, same shots): counts
        (B, S, K) for a state, (B, 4^n, S, K) for a process -> radii (B, len(conf_levels)).  One moment launch for the
        batch; the gamma / normal quantiles are SciPy's, vectorised over the batch."""
        dim, n_measurements, own, inv_matrix = self._design()
        c = np.asarray(counts)
        c = c.reshape((c.shape[0],) + own.shape)
        mean, variance = self._engine().moments(c, n_measurements, inv_matrix)
        distr = self._distribution(mean[:, None], variance[:, None])
        return np.sqrt(distr.ppf(np.asarray(conf_levels, dtype=np.float64)[None, :])) * self._alpha(dim)


def _distance_buffers(eng, n, centre):
    """On the engine's device: (dist float64 (n,), status int32 (n,) zeroed, `centre` as complex128)."""
    import torch

    dev = torch.device("cuda", eng.device)
    return (torch.empty(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
            torch.from_numpy(np.ascontiguousarray(centre, dtype=np.complex128)).to(dev))


# What a batch of resamples raises, in order of precedence: (status code -- None: any but 0 --, exception, text).
_STATE_ERRORS = ((1, np.linalg.LinAlgError, "starting point of the MLE is not positive definite"),
                 (_capi.TRIAL_SHOTS, ValueError, "per-setting totals of a trial do not match the registered shots"))
_PROCESS_ERRORS = ((None, ValueError, "a resampled process has no finite Choi matrix (an input state without counts)"),)


def _error_flags(status, errors):
    """Bool device tensor: which of `errors` the int32 `status` of a batch shows."""
    import torch

    flags = [(status != 0 if code is None else status == code).any() for code, _, _ in errors]
    return torch.stack(flags) if len(flags) > 1 else flags[0].reshape(1)  # (one flag: no launch of its own)


def _agreed_flags(bad):
    """This rank's `_error_flags` OR-ed over the ranks, as int64 on the host: every rank raises, or none.  One
    `allgather_equal` when there are several ranks -- a rank with an empty shard takes part with zeros."""
    bad = bad.cpu().numpy().astype(np.int64)
    if qdist.world()[1] > 1:
        bad = qdist.allgather_equal(bad).max(axis=0)
    return bad


def _raise_flagged(bad, errors):
    for flag, (_, kind, text) in zip(bad, errors):
        if flag:
            raise kind(text)


class _ShardedBootstrap:
    """What the one-pass bootstraps keep of their resamples: `boot_dist` and `boot_counts`, plain attributes on the
    two-pass paths, fetched from where `_setup_fused` left them on first use otherwise."""

    def _finish_fused(self, boot, eng, counts, dist, status, errors):
        """The end of a one-pass bootstrap, whose launches wrote this rank's `dist` and `status`: sync; the shard's
        `errors`, agreed over the ranks (`_agreed_flags`: one collective), are raised in order; sampler='device' on one
        rank leaves `boot` with the results of the last resample (`counts[-1]`), as the last experiment() would;
        `boot_dist` keeps the distances in resample order on the device (all-gathered when read); the shard is sorted
        where it is, and `cl_to_dist` evaluates interp1d's order statistics across the ranks (distributed.ShardedSample)
        -- no all-gather of the sample unless somebody reads `boot_dist` / `cl_to_dist.y`."""
        eng.sync()
        _raise_flagged(_agreed_flags(_error_flags(status, errors)), errors)
        if self.sampler == "device" and qdist.world()[1] == 1:
            boot.results = counts[-1].cpu().numpy()
        self._dist_shard, self._boot_dist = dist.clone(), None  # resample order; the sample below is sorted in place
        self.sample = qdist.ShardedSample(dist, self.n_points, engine=eng)
        self.cl_to_dist = _SampleInterp(self.sample)

    @property
    def boot_dist(self):
        """The distances in resample order, on the host (all-gathered on first use when the ranks hold shards)."""
        if getattr(self, "_boot_dist", None) is None and getattr(self, "_dist_shard", None) is not None:
            self._boot_dist = qdist.allgather_device(self._dist_shard, self.n_points).cpu().numpy()
        return getattr(self, "_boot_dist", None)

    @boot_dist.setter
    def boot_dist(self, value):
        self._boot_dist, self._dist_shard = value, None

    @property
    def boot_counts(self):
        """Every resample's counts on the host.  sampler='device': this rank's shard only (rows lo .. hi of the table),
        fetched when somebody reads it -- from the device tensor that holds it (states), or, where the shard was drawn
        and consumed chunk by chunk (processes), drawn again from the same Philox streams."""
        source = getattr(self, "_boot_counts_device", None)
        if getattr(self, "_boot_counts_host", None) is None and source is not None:
            self._boot_counts_host = source() if callable(source) else source.cpu().numpy()
        return getattr(self, "_boot_counts_host", None)

    @boot_counts.setter
    def boot_counts(self, value):
        self._boot_counts_host, self._boot_counts_device = value, None


class BootstrapStateInterval(_ShardedBootstrap, ConfidenceInterval):
    """Parametric bootstrap around `state` (default: the tomograph's reconstructed state) with the
    tomograph's own POVM and shots; distances tmg.dst(resampled estimate, state)."""

    _CHUNK_BYTES = 256 << 20  # density matrices of one chunk of resamples (trace distance / infidelity)

    def __init__(self, tmg, n_points=1000, method="lin", physical=True, init="lin", tol=1e-3, max_iter=100,
                 state=None, sampler="numpy", seed=None):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    def setup(self):
        if self.mode == Mode.CHANNEL:
            raise NotImplementedError("This interval works only for state tomography")
        tmg = self.tmg
        if self.state is None:
            if hasattr(tmg, "reconstructed_state"):
                self.state = tmg.reconstructed_state
            else:
                self.state = tmg.point_estimate(method=self.method, physical=self.physical, init=self.init,
                                                tol=self.tol, max_iter=self.max_iter)
        boot = tmg.__class__(self.state, tmg.dst)
        metric = _engine_metric(tmg.dst, self.state.n_qubits)
        if self.n_points and (tmg.dst is hs_dst or metric) and self.method in ("lin", "mle"):
            self._setup_fused(boot, metric)
            return
        # every resample's counts, one global RNG stream in the reference's order (resample after resample, setting
        # after setting): ONE call of the C restatement of NumPy's sampler instead of n_points x S Python calls
        # (sampler='device', opt-in: the same distribution drawn on the GPU, off the reference's stream)
        counts = boot.experiment_batch(tmg.n_measurements, tmg.povm_matrix, self.n_points, sampler=self.sampler,
                                       seed=self.seed)
        counts = qdist.broadcast_array(counts) if self.n_points else np.empty((0,) + tmg.results.shape)
        self.boot_counts = counts
        centre = self.state

        def reconstruct(shard):
            rho, info = boot.point_estimate_batch(shard, method=self.method, physical=self.physical, init=self.init,
                                                  tol=self.tol, max_iter=self.max_iter)
            if info is not None and np.any(info["status"] == 1):
                raise np.linalg.LinAlgError("starting point of the MLE is not positive definite")
            if tmg.dst is hs_dst:
                return get_engine(centre.n_qubits).distance(rho, centre.matrix)
            from ..qobj import Qobj

            return np.array([tmg.dst(Qobj(r), centre) for r in rho], dtype=np.float64)

        self.boot_dist = qdist.sharded_map(counts, reconstruct)
        self._finish(self.boot_dist)

    def _setup_fused(self, boot, metric=None):
        """The loop of interval.py:598-609 for the Hilbert-Schmidt distance and the 'lin' / 'mle' estimators, as this
        rank's shard of it: the shard's counts go to (sampler='numpy': one C call on np.random's stream on rank 0,
        broadcast) or are drawn in (sampler='device': row resample * S + setting of the table keyed by `shared_seed`,
        each rank draws only its own: `device_chunks`, the shard as one chunk) HBM, ONE launch family reconstructs them
        and writes the distance to `state` (qt_lin_dist_batch / qt_mle_dist_batch: 8 bytes per resample leave the
        kernel, no density matrices), and `_finish_fused` ends the pass.
        `metric` = 'trace' / 'if': the same, except that the shard is reconstructed in chunks of whole
        trials into a workspace of at most `_CHUNK_BYTES` of density matrices, and `Engine.distance_dev` writes each
        chunk's trace distances / infidelities to `state` into the shard's `dist`: the matrices never leave HBM."""
        import torch

        tmg = self.tmg
        lo, hi = qdist.shard_bounds(self.n_points)
        povm_matrix, shots, pvals = boot._experiment_tables(tmg.n_measurements, tmg.povm_matrix)
        boot.povm_matrix, boot.n_measurements = povm_matrix, np.asarray(shots)
        eng = boot._engine()
        dev = torch.device("cuda", eng.device)
        n_set, n_out = pvals.shape
        d = 2 ** self.state.n_qubits
        if self.sampler == "device":
            check_pvals(pvals)
            seed = shared_seed(self.seed)
            counts = torch.empty((0, n_set, n_out), dtype=torch.int64, device=dev)
            for _, counts in device_chunks(eng, shots, pvals, n_set, lo, hi, hi - lo, seed, (n_set, n_out)):
                pass  # the whole shard is one chunk: `boot_counts` reads it
            self._boot_counts_host, self._boot_counts_device = None, counts
        elif self.sampler == "numpy":
            host = boot.experiment_batch(tmg.n_measurements, tmg.povm_matrix, self.n_points) if qdist.world()[0] == 0 else \
                np.empty((self.n_points, n_set, n_out), dtype=np.int64)
            self.boot_counts = qdist.broadcast_array(host)
            counts = torch.from_numpy(np.ascontiguousarray(self.boot_counts[lo:hi])).to(dev)
        else:
            raise ValueError(f"sampler must be 'numpy' or 'device', not {self.sampler!r}")
        dist, status, centre = _distance_buffers(eng, hi - lo, self.state.matrix)
        if hi > lo and metric is None:
            if self.method == "lin":
                eng.lin_dist_dev(counts, centre, dist, physical=self.physical, status=status)
            else:
                eng.mle_dist_dev(counts, centre, dist, init=self.init, max_iter=self.max_iter, tol=self.tol, status=status)
        elif hi > lo:
            chunk = min(hi - lo, max(1, self._CHUNK_BYTES // (16 * d * d)))
            rho = torch.empty((chunk, d, d), dtype=torch.complex128, device=dev)
            for c0 in range(0, hi - lo, chunk):
                c1 = min(c0 + chunk, hi - lo)
                if self.method == "lin":
                    eng.lin_dev(counts[c0:c1], rho[:c1 - c0], physical=self.physical, status=status[c0:c1])
                else:
                    eng.mle_dev(counts[c0:c1], rho[:c1 - c0], init=self.init, max_iter=self.max_iter, tol=self.tol,
                                status=status[c0:c1])
                eng.distance_dev(rho[:c1 - c0], centre, dist[c0:c1], metric)
        self._finish_fused(boot, eng, counts, dist, status, _STATE_ERRORS)


class _SampleInterp:
    """`interp1d(np.linspace(0, 1, n), sorted_dist)` (interval.py:611-612) over a `ShardedSample`: calling it evaluates
    the order statistics where the shards are (collective when there are several ranks); `.x` / `.y` are interp1d's
    attributes, `.y` gathering the sorted sample on first use."""

    def __init__(self, sample):
        self.sample = sample

    def __call__(self, conf_levels):
        cl = np.asarray(conf_levels, dtype=np.float64)
        return self.sample.quantiles(cl.reshape(-1)).reshape(cl.shape)

    @property
    def y(self):
        full = self.sample.gather_sorted()
        if not isinstance(full, np.ndarray):
            self.sample.engine.sync()
            full = full.cpu().numpy()
        return full

    @property
    def x(self):
        return np.linspace(0, 1, self.sample.n_total)


class _ChainInterval(ConfidenceInterval):
    """The chain set-up of both MHMC intervals.  A subclass names the start point (`_start`), the engine's chain
    (`_CHAIN`) and what a kept chain state is (`_kept`)."""

    def _sample_distances(self, eng, dim, centre, metric):
        """One run of the chain in `dim` real parameters -> the distances of its samples to `centre`, unsorted.
        `_x_t` is the state the next run continues from, `_burned` whether the burn-in is behind it; without
        `warm_start` (or on the first run) the chain starts at `_start` and burns in.  The random numbers are drawn as
        the reference draws them (`_proposal_increments`, then `numpy.random.rand`: increments before uniforms, the
        burn-in's before the samples') and the whole run is ONE launch of `_CHAIN`.  Sets `samples` (every
        `thinning`-th state behind the burn-in) and `acceptance_rate` (the accepted share of the steps behind it)."""
        tmg = self.tmg
        if not (self.warm_start and hasattr(self, "_x_t")):
            self._x_t, self._burned = self._start(eng, centre), False
        jump = _proposal_increments(dim)
        total = self.n_points * self.thinning
        skip = 0 if self._burned else self.burn_steps
        parts = [(jump(steps), np.random.rand(steps)) for steps in ([total] if self._burned else [skip, total])]
        deltas, uniforms = (np.concatenate(part) for part in zip(*parts))
        chain, accepted = getattr(eng, self._CHAIN)(tmg.results, self._x_t, deltas, uniforms, self.step)
        self._burned = True
        if len(chain):
            self._x_t = chain[-1].copy()
        self.samples, mats = self._kept(eng, chain[skip::self.thinning][: self.n_points])
        self.acceptance_rate = float(accepted[skip:].mean()) if total else 0.0
        if tmg.dst is hs_dst or metric:
            return eng.distance(mats, centre, metric)
        return np.array([tmg.dst(m, centre) for m in mats], dtype=np.float64)


class MHMCStateInterval(_ChainInterval):
    """Metropolis-Hastings samples of the likelihood on the Cholesky parameters around the point estimate
    (reference interval.py:689-750, mhmc.py): distances tmg.dst(sample, state), sorted.  The random numbers are
    drawn on the host in the reference's order (`_ChainInterval`); the chain itself (one likelihood evaluation per
    step, inherently serial) runs in one launch of `qt_mhmc_state`, for n = 1 .. 5 qubits (n = 4, 5: one workgroup
    per chain)."""

    def __init__(self, tmg, n_points=1000, step=0.01, burn_steps=1000, thinning=1, warm_start=False,
                 use_new_estimate=False, state=None, verbose=False):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    _CHAIN = "mhmc_state"

    def _start(self, eng, centre):
        x0, status = eng.chol_param(centre)
        if status == 1:  # the reference fails inside scipy.linalg.cholesky here
            raise np.linalg.LinAlgError("the state the chain starts from is not positive definite")
        return x0

    def _kept(self, eng, chain):
        return chain, eng.chol_unparam(chain)  # samples: Cholesky parameters; measured: their density matrices

    def setup(self):
        if self.mode == Mode.CHANNEL:
            raise NotImplementedError("This interval works only for state tomography")
        tmg = self.tmg
        if not self.use_new_estimate:
            self.state = tmg.reconstructed_state
        elif self.state is None:
            self.state = tmg.point_estimate(method="mle", physical=True)
        centre = np.asarray(self.state.matrix, dtype=np.complex128)
        self._finish(self._sample_distances(tmg._engine(), 4**tmg.state.n_qubits, centre,
                                            _engine_metric(tmg.dst, tmg.state.n_qubits)))


class SugiyamaInterval(ConfidenceInterval):
    """Hoeffding-type interval of Sugiyama et al., arXiv:1306.4191 (reference interval.py:219-265): closed
    form in the left inverse of the rescaled POVM matrix (computed on the GPU, `qt_left_inverse`)."""

    def __init__(self, tmg, n_points=1000, max_confidence=0.999):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    def setup(self):
        if self.mode == Mode.CHANNEL:
            raise NotImplementedError("Sugiyama interval works only for state tomography")
        tmg = self.tmg
        dim = 2**tmg.state.n_qubits
        dist = np.linspace(0, 1, self.n_points)
        settings, outcomes, width = tmg.povm_matrix.shape
        scaled = np.reshape(np.asarray(tmg.povm_matrix), (-1, width)) * dim / np.sqrt(2 * dim)
        inverse = get_engine(tmg.state.n_qubits).left_inverse_of(scaled).reshape(-1, settings, outcomes)
        ratios = tmg.n_measurements.sum() / tmg.n_measurements
        spread = np.max(inverse, axis=-1) - np.min(inverse, axis=-1)
        c_alpha = np.sum(spread**2 * ratios[None, :], axis=-1) + self.EPS
        if tmg.dst == hs_dst:
            b = 8 / (dim**2 - 1)
        elif tmg.dst == trace_dst:
            b = 16 / (dim**2 - 1) / dim
        elif tmg.dst == if_dst:
            b = 4 / (dim**2 - 1) / dim
        else:
            raise NotImplementedError("Unsupported distance")
        conf_levels = 1 - 2 * np.sum(np.exp(-b * dist[:, None] ** 2 * np.sum(tmg.n_measurements) / c_alpha[None, :]),
                                     axis=1)
        self.cl_to_dist = interp1d(conf_levels, dist)


class HolderInterval(ConfidenceInterval):
    """Process interval assembled from one state interval per input state (reference interval.py:421-539):
    conf_level^(number of inputs) and sqrt(sum_ij |c_i . conj(c_j)| delta_i delta_j) over the
    coordinates c of the single-entry matrices in the input basis.  `kind` in {'mhmc', 'bootstrap',
    'sugiyama'}; as in the reference, the default 'wang' (and 'boot') is rejected by `setup` with a
    ValueError and 'moment' fails on MomentInterval's signature."""

    def __init__(self, tmg, n_points=1000, kind="wang", max_confidence=0.999, method="lin", method_boot="lin",
                 physical=True, init="lin", tol=1e-3, max_iter=100, step=0.01, burn_steps=1000, thinning=1):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    def __call__(self, conf_levels=None):
        conf_levels = _levels_or_default(conf_levels)
        if not hasattr(self, "intervals"):
            self.setup()
        results = [interval(conf_levels) for interval in self.intervals]
        deltas = np.asarray([r[0] for r in results])
        conf_levels = results[0][1] ** self.tmg.input_basis.dim
        entries = self.tmg._decomposed_single_entries
        coef = np.abs(np.einsum("ij,ik->jk", entries, entries.conj()))
        dist = np.sqrt(np.einsum("ik,jk,ij->k", deltas, deltas, coef))
        return dist, conf_levels

    def setup(self):
        if self.mode == Mode.STATE:
            raise NotImplementedError("Holder interval works only for process tomography")
        parts = self.tmg.tomographs
        if self.kind == "moment":
            self.intervals = [MomentInterval(t, self.n_points, self.max_confidence) for t in parts]  # TypeError, as there
        elif self.kind == "mhmc":
            self.intervals = [MHMCStateInterval(t, self.n_points, self.step, self.burn_steps, self.thinning) for t in parts]
        elif self.kind == "bootstrap":
            self.intervals = [BootstrapStateInterval(t, self.n_points, self.method, physical=self.physical, init=self.init,
                                                     tol=self.tol, max_iter=self.max_iter) for t in parts]
        elif self.kind == "sugiyama":
            self.intervals = [SugiyamaInterval(t, self.n_points, self.max_confidence) for t in parts]
        else:
            raise ValueError("Incorrect value for argument `kind`.")
        for interval in self.intervals:
            interval.setup()


def count_confidence(delta, frequencies, n_measurements):
    """Confidence level of the polytope of frequencies widened by `delta` (reference polytopes/utils.py:4-15): the
    product over settings of max(1 - sum over outcomes of exp(-n_s KL(f || clip(f + delta))), 0), with the
    divergence +inf where the clip reaches its top and the term 0 for a frequency of 1."""
    eps = 1e-15
    f = np.asarray(frequencies, dtype=np.float64)
    shifted = np.clip(f + delta, eps, 1 - eps)
    kl = f * np.log(f / shifted) + (1 - f) * np.log((1 - f) / (1 - shifted))
    kl = np.where(shifted < 1 - eps, kl, np.inf)
    eps_k = np.exp(-np.asarray(n_measurements)[:, None] * kl)
    eps_k = np.where(np.abs(f - 1) < 2 * eps, 0, eps_k)
    return np.prod(np.maximum(1 - np.sum(eps_k, axis=-1), 0))


def count_delta(target_cl, frequencies, n_measurements):
    """The widening whose confidence level is `target_cl` (reference polytopes/utils.py:18-27): bisection on
    [1e-10, 1] down to a width of 1e-10, the left end moving while the level is below target + 1e-10; the last
    midpoint is returned."""
    left, right = 1e-10, 1.0
    delta = None
    while right - left > 1e-10:
        delta = (left + right) / 2
        if count_confidence(delta, frequencies, n_measurements) < target_cl + 1e-10:
            left = delta
        else:
            right = delta
    return delta


def _state_only(interval, name):
    if interval.mode == Mode.CHANNEL:
        raise NotImplementedError(f"{name} works only for state tomography")


def _objective_or_one(value, to_fidelity):
    """The reference's `if not sol["primal objective"]: 1` (interval.py:146-153, :313-322): a missing optimum
    (cvxopt's None for an infeasible or unbounded program) and an optimum of exactly 0.0 both give 1."""
    value = np.asarray(value, dtype=np.float64)
    return np.where(np.isfinite(value) & (value != 0.0), to_fidelity(value), 1.0)


class _FidelityBounds:
    """A two-sided interval: `interval(conf_levels)` -> ((lower bounds, upper bounds), conf_levels), interpolated in the
    table `_tabulate` leaves (`conf_levels`, `dist_min`, `dist_max`, `cl_to_dist_min`, `cl_to_dist_max`)."""

    def __call__(self, conf_levels=None):
        conf_levels = _levels_or_default(conf_levels)
        if not hasattr(self, "cl_to_dist_max"):
            self.setup()
        return (self.cl_to_dist_min(conf_levels), self.cl_to_dist_max(conf_levels)), conf_levels

    def _tabulate(self, conf_levels, dist_min, dist_max):
        self.conf_levels, self.dist_min, self.dist_max = conf_levels, dist_min, dist_max
        self.cl_to_dist_min = interp1d(conf_levels, dist_min)
        self.cl_to_dist_max = interp1d(conf_levels, dist_max)

    def _tabulate_polytope(self, lp, deltas, frequencies, shots, to_min, to_max):
        """The end of a polytope interval's setup(): lp = (objectives (n_points, 2) of min c . x and min -c . x, status,
        iterations) at `deltas`.  A program that did not converge raises; the bounds are to_min / to_max of the
        objectives through `_objective_or_one`, the level of a widening is `count_confidence(delta)`."""
        obj, status, iters = lp
        bad = np.flatnonzero((status == _capi.LP_NOT_CONVERGED).any(axis=1))
        if bad.size:
            raise RuntimeError(f"the interior-point LP solver did not converge at delta index {bad[:8].tolist()}")
        self.deltas, self.lp_status, self.lp_iters = deltas, status, iters
        shots = np.asarray(shots, dtype=np.float64)
        self._tabulate(np.array([count_confidence(d, frequencies, shots) for d in deltas]),
                       _objective_or_one(obj[:, 0], to_min), _objective_or_one(obj[:, 1], to_max))


class MomentFidelityStateInterval(_FidelityBounds, MomentInterval):
    """Fidelity bounds with a target state from the moment interval's radii (reference interval.py:113-160).

    For every level of a fixed 280-point grid the reference solves two SOCPs with cvxopt: minimise (maximise)
    target.bloch . x over Bloch vectors x with x_0 = 1 / d and ||x - x_hat|| <= radius * sqrt(2 / d), x_hat being the
    tomograph's (unconstrained) linear-inversion estimate.  That program is a linear objective over a ball cut by a
    hyperplane, whose optimum is closed-form: c_0 / d + c' . x_hat' -+ rho ||c'|| with rho^2 = R^2 - (x_hat_0 - 1/d)^2
    (primes drop index 0); an empty cut (rho^2 < 0) and an optimum of exactly 0.0 give 1, as the reference's
    `if not sol["primal objective"]` does.  The bounds are not clipped to [0, 1] (the reference clips only in its
    command-line script).

    Deviation: a process tomograph raises NotImplementedError in __init__ (the reference fails later, in setup)."""

    def __init__(self, tmg, distr_type="gamma", target_state=None):
        super().__init__(tmg, distr_type=distr_type)
        self.target_state = target_state
        _state_only(self, "MomentFidelityStateInterval")

    @staticmethod
    def levels():
        """The reference's grid of confidence levels (interval.py:131)."""
        return np.concatenate((np.arange(1e-7, 0.8, 0.01), np.linspace(0.8, 1 - 1e-7, 200)))

    def setup(self):
        super().setup()
        tmg = self.tmg
        if not hasattr(tmg, "reconstructed_state"):
            tmg.point_estimate(physical=False)
        if self.target_state is None:
            self.target_state = tmg.reconstructed_state
        dim = 2**tmg.state.n_qubits
        conf_levels = self.levels()
        radius = np.asarray(self.cl_to_dist(conf_levels), dtype=np.float64) * np.sqrt(2 / dim)
        c = np.asarray(self.target_state.bloch, dtype=np.float64)
        x_hat = np.asarray(tmg.reconstructed_state.bloch, dtype=np.float64)
        rho2 = radius**2 - (x_hat[0] - 1 / dim) ** 2
        rho = np.sqrt(np.maximum(rho2, 0.0))
        centre = c[0] / dim + c[1:] @ x_hat[1:]
        norm = np.linalg.norm(c[1:])
        low = np.where(rho2 >= 0, centre - rho * norm, np.nan)     # min c . x
        high = np.where(rho2 >= 0, -centre - rho * norm, np.nan)   # min -c . x
        self._tabulate(conf_levels, _objective_or_one(low, lambda v: v * dim), _objective_or_one(high, lambda v: -v * dim))


class PolytopeStateInterval(_FidelityBounds, ConfidenceInterval):
    """Fidelity bounds with a target state from a polytope of states (Kiktenko et al., arXiv:2109.04734; reference
    interval.py:268-335).

    For n_points widenings delta between count_delta(0) and count_delta(1 - 1e-7) the Bloch vectors whose outcome
    probabilities lie within clip(f + delta) form a polytope A x <= b(delta); the fidelity bounds at confidence level
    count_confidence(delta) are 1/d + d min(c . x) and 1/d - d min(-c . x) over it, c = target.bloch[1:].  The
    reference makes 2 * n_points cvxopt `solvers.lp` calls; here all of them are one launch of the batched
    interior-point solver (qt_lp_ineq_batch, n <= 3 qubits).  As in the reference an infeasible or unbounded program,
    and an optimum of exactly 0.0 (always the case for c = 0, e.g. the maximally mixed target), give 1.  A program that
    does not converge raises.  A POVM that is not informationally complete (rank of A below 4^n - 1) raises ValueError
    before any launch, as cvxopt's `lp` does on such a G.

    Deviation: a process tomograph raises NotImplementedError in __init__ (the reference raises it in setup)."""

    _MAX_QUBITS, _MAX_VARIABLES = 3, 64  # polytopes.StateFidelityInterval goes to n = 4 on the second LP kernel

    def __init__(self, tmg, n_points=1000, target_state=None):
        super().__init__(tmg, **_pop_hidden_keys(locals()))
        _state_only(self, type(self).__name__)

    def _lp(self, A, C, b):
        return get_engine(self.tmg.state.n_qubits).lp_ineq_batch(A, C, b)

    def programs(self):
        """(A, b (n_points, M), c, deltas, frequencies) of the reference's LPs (interval.py:297-316)."""
        tmg = self.tmg
        n_qubits = tmg.state.n_qubits
        if n_qubits > self._MAX_QUBITS:
            raise NotImplementedError(f"{type(self).__name__} supports n <= {self._MAX_QUBITS} qubits (4^n - 1 <= "
                                      f"{self._MAX_VARIABLES} LP variables); got n = {n_qubits}")
        dim = 2**n_qubits
        shots = np.asarray(tmg.n_measurements, dtype=np.float64)
        frequencies = np.clip(np.asarray(tmg.results) / shots[:, None], self.EPS, 1 - self.EPS)
        povm = np.asarray(tmg.povm_matrix, dtype=np.float64)
        weighted = np.reshape(povm * shots[:, None, None] / np.sum(shots), (-1, povm.shape[-1])) * povm.shape[0]
        A = np.ascontiguousarray(weighted[:, 1:]) * dim
        if np.linalg.matrix_rank(A) < A.shape[1]:
            raise ValueError("Rank(A) < size(x): the POVM is not informationally complete")
        c = np.asarray(self.target_state.bloch, dtype=np.float64)[1:]
        deltas = np.linspace(count_delta(0, frequencies, shots), count_delta(1 - 1e-7, frequencies, shots), self.n_points)
        b = np.clip(np.ravel(frequencies)[None, :] + deltas[:, None], self.EPS, 1 - self.EPS) - weighted[None, :, 0]
        return A, b, c, deltas, frequencies

    def setup(self):
        tmg = self.tmg
        if self.target_state is None:
            self.target_state = tmg.state
        dim = 2**tmg.state.n_qubits
        A, b, c, deltas, frequencies = self.programs()
        self._tabulate_polytope(self._lp(A, np.stack([c, -c]), b), deltas, frequencies, tmg.n_measurements,
                                lambda v: 1 / dim + v * dim, lambda v: 1 / dim - v * dim)


def _needs_cvxopt(name, lines, see=""):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError(f"{name} (reference interval.py:{lines}) poses a cone / linear program for cvxopt; "
                                  f"that solver is outside the tomography hot path and is not provided{see}")

    return type(name, (ConfidenceInterval,), {"__init__": __init__, "setup": lambda self: None,
                                              "__doc__": f"Placeholder: the reference's {name} needs cvxopt{see or '.'}"})


MomentFidelityProcessInterval = _needs_cvxopt("MomentFidelityProcessInterval", "163-216")
PolytopeProcessInterval = _needs_cvxopt(
    "PolytopeProcessInterval", "338-418",
    ".  The same fidelity bounds, from the batched GPU LP solver, are quantpy_amd.tomography.polytopes.ProcessFidelityInterval.")


class MHMCProcessInterval(_ChainInterval):
    """Metropolis-Hastings samples of the process likelihood on the Choi vector (reference
    interval.py:763-850): every proposal x + step * delta is projected onto the CPTP set
    (`_cptp_update_rule`, process.py:279-281), the target is exp(-nll) with the raw counts.  Draws on the
    host in the reference's order, the chain in one launch of `qt_mhmc_process`.  As in the reference,
    `return_samples=True` makes `setup()` return (dist, conf_levels, acceptance_rate, matrices) instead of
    preparing the functor."""

    def __init__(self, tmg, n_points=1000, step=0.01, burn_steps=1000, thinning=1, warm_start=False, method="lifp",
                 states_est_method="lin", states_physical=True, states_init="lin", use_new_estimate=False,
                 channel=None, verbose=False, return_samples=False):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    _CHAIN = "mhmc_process"

    def _start(self, eng, centre):
        return centre.copy()

    def _kept(self, eng, chain):
        # mhmc.py:66 collects the samples in a REAL array: the imaginary parts of the chain states are
        # dropped there (NumPy's ComplexWarning), and the distances are those of the real parts
        real = np.ascontiguousarray(chain.real)
        return real, real

    def setup(self):
        if self.mode == Mode.STATE:
            raise NotImplementedError("This interval works only for process tomography")
        tmg = self.tmg
        if not self.use_new_estimate:
            self.channel = tmg.reconstructed_channel
        elif self.channel is None:
            self.channel = tmg.point_estimate(self.method, states_est_method=self.states_est_method,
                                              states_physical=self.states_physical, states_init=self.states_init)
        centre = np.asarray(self.channel.choi.matrix, dtype=np.complex128)
        # trace distance / infidelity of the Choi matrices, 2n-qubit objects: on the engine (dim 4, 16, 64); the real
        # parts of Hermitian chain states are symmetric, hence Hermitian, which is what metric_dist takes
        metric = _engine_metric(tmg.dst, 2 * self.channel.n_qubits, max_qubits=6)
        dist = np.sort(self._sample_distances(tmg._engine(), 16**tmg.channel.n_qubits, centre, metric))
        conf_levels = np.linspace(0, 1, len(dist))
        if self.return_samples:
            return dist, conf_levels, self.acceptance_rate, list(self.samples)
        self.cl_to_dist = interp1d(conf_levels, dist)


class BootstrapProcessInterval(_ShardedBootstrap, ConfidenceInterval):
    """Parametric bootstrap of a process tomography around `channel` (default: the reconstructed
    channel): resampled counts for every input state, batched Choi reconstruction.

    method='lifp' with the Hilbert-Schmidt distance runs in one pass per rank (`_setup_fused`); with sampler='device'
    the counts then never leave the GPU: `boot_counts` is this rank's shard, drawn again from the same streams when it
    is read.  `chunk` (keyword-only) overrides how many resamples of the shard are drawn and reconstructed at a time
    (default: 256 MB of counts); the draws and distances do not depend on it."""

    _CHUNK_BYTES = 256 << 20

    def __init__(self, tmg, n_points=1000, method="lifp", cptp=True, tol=1e-10, channel=None,
                 states_est_method="lin", states_physical=True, states_init="lin", sampler="numpy", seed=None, *,
                 chunk=None):
        super().__init__(tmg, **_pop_hidden_keys(locals()))

    def setup(self):
        if self.mode == Mode.STATE:
            raise NotImplementedError("This interval works only for process tomography")
        tmg = self.tmg
        if self.channel is None:
            if hasattr(tmg, "reconstructed_channel"):
                self.channel = tmg.reconstructed_channel
            else:
                self.channel = tmg.point_estimate(method=self.method, states_physical=self.states_physical,
                                                  states_init=self.states_init, cptp=self.cptp)
        boot = tmg.__class__(self.channel, tmg.input_states, tmg.dst)
        shots, povm = tmg.tomographs[0].n_measurements, tmg.tomographs[0].povm_matrix
        if self.n_points and tmg.dst is hs_dst and self.method == "lifp":
            self._setup_fused(boot, shots, povm)
            return
        counts = qdist.broadcast_array(boot.experiment_batch(shots, povm=povm, repeats=self.n_points,
                                                             sampler=self.sampler, seed=self.seed))
        self.boot_counts = counts
        centre = self.channel.choi
        # trace distance / infidelity of the Choi matrices on the engine (dim 4, 16, 64), as MHMCProcessInterval measures
        # its samples
        metric = _engine_metric(tmg.dst, 2 * tmg.channel.n_qubits, max_qubits=6)

        def reconstruct(shard):
            # the reference's loop (interval.py:675-680) passes method, states_physical, states_init and cptp;
            # `tol` and `states_est_method` stay at point_estimate's defaults there, and so they do here
            choi = boot.point_estimate_batch(shard, method=self.method, cptp=self.cptp,
                                             states_physical=self.states_physical, states_init=self.states_init)
            if tmg.dst is hs_dst or metric:  # 4^n x 4^n matrices on the channel's engine
                return get_engine(tmg.channel.n_qubits).distance(choi, centre.matrix, metric)
            from ..qobj import Qobj

            return np.array([tmg.dst(Qobj(c), centre) for c in choi], dtype=np.float64)

        self.boot_dist = qdist.sharded_map(counts, reconstruct)
        self._finish(self.boot_dist)

    def _setup_fused(self, boot, shots, povm):
        """The loop of interval.py:673-682 for 'lifp' and the Hilbert-Schmidt distance as this rank's shard of it, the way
        BootstrapStateInterval._setup_fused runs the state loop: the shard's counts go to (sampler='numpy': drawn on
        np.random's stream on rank 0, broadcast) or are drawn in (sampler='device': row (resample * 4^n + input) * S +
        setting of the table keyed by that global index, `ProcessTomograph.experiment_batch`'s keying, so each rank
        draws only its own rows) HBM, qt_lifp_dist_batch reconstructs them and writes the distance to `channel` -- 8
        bytes per resample leave the kernels, no Choi matrices -- and `_finish_fused` ends the pass.  The device
        sampler's shard is drawn and consumed `chunk` resamples at a time (`device_chunks`: the chunking changes no
        draw).  As in the reference's loop, `cptp` is passed on and `tol` is not."""
        import torch

        lo, hi = qdist.shard_bounds(self.n_points)
        if self.sampler == "numpy":
            if self.seed is not None:  # (every rank: what draw_counts tells rank 0)
                raise ValueError("sampler='numpy' draws from np.random's global stream: seed it with np.random.seed")
            if qdist.world()[0] == 0:
                host = boot.experiment_batch(shots, povm=povm, repeats=self.n_points)
            else:
                povm_matrix, shots_set, probas = boot._experiment_tables(shots, povm)
                host = np.empty((self.n_points, len(boot.tomographs), povm_matrix.shape[0], probas.shape[1]), dtype=np.int64)
            self.boot_counts = host = qdist.broadcast_array(host)
            n_in, n_set, n_out = host.shape[1:]
        elif self.sampler == "device":
            povm_matrix, shots_set, probas = boot._experiment_tables(shots, povm)
            n_in = len(boot.tomographs)
            n_set, n_out = probas.shape[0] // n_in, probas.shape[1]
            check_pvals(probas)
            seed = shared_seed(self.seed)
            shots_rows = np.tile(np.asarray(shots_set).astype(np.int64), n_in)
        else:
            raise ValueError(f"sampler must be 'numpy' or 'device', not {self.sampler!r}")
        if not hasattr(boot.tomographs[0], "povm_matrix"):  # (no experiment_batch on this rank) what the engine's set-up reads
            for t in boot.tomographs:
                t.povm_matrix, t.n_measurements = povm_matrix, np.asarray(shots_set)
        eng = boot._engine()
        rows = n_in * n_set  # table rows per resample
        dist, status, centre = _distance_buffers(eng, hi - lo, self.channel.choi.matrix)
        counts = None
        if self.sampler == "numpy" and hi > lo:
            counts = torch.from_numpy(np.ascontiguousarray(host[lo:hi])).to(dist.device)
            eng.lifp_dist_dev(counts, centre, dist, cptp=self.cptp, status=status)
        elif self.sampler == "device":
            chunk = int(self.chunk) if self.chunk else max(1, self._CHUNK_BYTES // (rows * n_out * 8))
            # one stream: a chunk's draw waits for the reconstruction before it
            for c0, counts in device_chunks(eng, shots_rows, probas, rows, lo, hi, chunk, seed, (n_in, n_set, n_out)):
                c1 = c0 + counts.shape[0]
                eng.lifp_dist_dev(counts, centre, dist[c0 - lo: c1 - lo], cptp=self.cptp, status=status[c0 - lo: c1 - lo])
            self._boot_counts_host = None
            self._boot_counts_device = lambda: (
                eng.device_multinomial(shots_rows, probas, (hi - lo) * rows, seed, first_row=lo * rows) if hi > lo else
                np.empty((0, n_out), dtype=np.int64)).reshape(hi - lo, n_in, n_set, n_out)
        self._finish_fused(boot, eng, counts, dist, status, _PROCESS_ERRORS)
