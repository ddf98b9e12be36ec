"""NumPy-facing wrapper of the C ABI (include/qtomo.h): one `Engine` per (n_qubits, device).

Every method is a thin marshalling layer over one `qt_*` entry point -- the arithmetic is in the
HIP kernels.  Inputs are NumPy arrays (host-pointer calls, synchronous) or torch CUDA tensors
(device-pointer calls, asynchronous on the engine's stream; outputs must then be passed in).
"""
import ctypes
import os
import sys

import numpy as np

from . import _capi

_STATUS_TEXT = {
    _capi.TRIAL_NOT_PD: "matrix is not positive definite (Cholesky)",
    _capi.TRIAL_LINESEARCH: "line search failed (precision loss)",
    _capi.TRIAL_MAXITER: "maximum number of iterations reached",
    _capi.TRIAL_NAN: "NaN encountered",
    _capi.TRIAL_SHOTS: "per-setting totals of the counts differ from the shots registered with set_povm",
}


def _check_shots(status):
    """The reference derives the weights N_s / sum N from each trial's own results (state.py:138-141, 194-197); the
    engine registers them once per POVM, so counts measured with other shot numbers must not pass silently."""
    bad = np.flatnonzero(np.asarray(status) == _capi.TRIAL_SHOTS)
    if bad.size:
        raise ValueError(f"counts of trial(s) {bad[:8].tolist()}{'...' if bad.size > 8 else ''}: per-setting totals are not "
                         "proportional to the n_measurements registered with set_povm (reconstruct them with their own "
                         "tomograph / set_povm call)")


def _torch_stream_ptr(device):
    """hipStream_t of torch's current stream on `device`, as an integer (0 = the legacy default stream)."""
    import torch

    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return int(raw(device))
    return int(torch.cuda.current_stream(device).cuda_stream)


class EngineError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libqtomo error {code}: {text}")
        self.code = code


def _is_dev(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _ptr(x):
    if x is None:
        return None
    if _is_dev(x):
        assert x.is_cuda and x.is_contiguous()
        return ctypes.c_void_p(x.data_ptr())
    return x.ctypes.data_as(ctypes.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def _i64(a):
    a = np.asarray(a)
    if a.dtype != np.int64:
        if not np.issubdtype(a.dtype, np.integer):
            if not np.all(np.equal(np.mod(a, 1), 0)):
                raise TypeError("counts must be integers")
        a = a.astype(np.int64)
    return np.ascontiguousarray(a)


_DEFAULT_DEVICE = None  # (LOCAL_RANK string, device index): resolved once per process (see default_device)


def default_device():
    """The device index an engine is created on when the caller names none: the process's own GPU.
    `QTOMO_DEVICE` if set; else torch's current device when the caller has moved it off device 0
    (`torch.cuda.set_device(local_rank)`: one rank per GPU); else `LOCAL_RANK` (torchrun) modulo the number of
    VISIBLE devices (a launcher that masks each rank down to one GPU with HIP_VISIBLE_DEVICES leaves LOCAL_RANK = 3
    pointing at device 0), resolved once per process -- so that torch initialising the GPU half-way through a run
    (current device 0 by default) does not move a rank's engines onto GPU 0; else 0."""
    global _DEFAULT_DEVICE
    env = os.environ.get("QTOMO_DEVICE")
    if env is not None:
        return int(env)
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        cur = int(torch.cuda.current_device())
        if cur != 0 or os.environ.get("LOCAL_RANK") is None:
            return cur
    lr = os.environ.get("LOCAL_RANK")
    if _DEFAULT_DEVICE is None or _DEFAULT_DEVICE[0] != lr:
        if lr is None:
            _DEFAULT_DEVICE = (lr, 0)
        else:
            n = _capi.load().qt_device_count()
            _DEFAULT_DEVICE = (lr, int(lr) % n if n > 0 else int(lr))
    return _DEFAULT_DEVICE[1]


class Engine:
    """Owns a qt_handle (device buffers, stream, cached POVM operators) for `n_qubits`.

    Host-pointer (NumPy) calls are synchronous.  Device-pointer (`*_dev`, torch tensors) calls are
    asynchronous on the handle's stream; each of them first makes sure the handle runs on torch's
    CURRENT stream of its device (re-binding when the caller has switched streams since the last call),
    so that they are ordered with the torch work that produced their inputs and consumes their
    outputs.  `stream="own"` keeps a private non-blocking stream instead (the caller then orders
    producers / consumers itself: `sync()`); an explicit `set_stream()` pins the handle likewise."""

    def __init__(self, n_qubits, device=None, stream="torch"):
        self.lib = _capi.load()
        self.n = int(n_qubits)
        self.d = 2**self.n
        self.D = 4**self.n
        self.device = default_device() if device is None else int(device)
        self._h = self.lib.qt_create(self.device, self.n)
        if not self._h:
            raise _capi.EngineUnavailable(_capi.last_error())
        self._povm_key = None
        self._proc_key = None
        self._stream_policy = stream  # "torch": follow torch's current stream; "own" / "pinned": leave the handle's stream alone
        self._bound_ptr = None        # the torch stream pointer the handle was last bound to
        self.S = self.K = self.M = 0

    def close(self):
        if getattr(self, "_h", None):
            self.lib.qt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, code):
        if code < 0:
            raise EngineError(code, _capi.last_error())
        return code

    # ---- plumbing ---------------------------------------------------------------------------
    def sync(self):
        self._chk(self.lib.qt_sync(self._h))

    def set_stream(self, stream_ptr):
        """Pin the handle to a hipStream_t given as an integer; 0 / None = a private stream, 1 = the legacy default
        stream.  Device-pointer calls stop following torch's current stream (`follow_torch_stream()` resumes that)."""
        self._chk(self.lib.qt_set_stream(self._h, ctypes.c_void_p(stream_ptr or None)))
        self._stream_policy = "pinned"
        self._bound_ptr = None

    def follow_torch_stream(self):
        self._stream_policy = "torch"
        self._bound_ptr = None

    def bind_torch_stream(self):
        """Run this engine's work on torch's current stream of its device (stream 0 = the legacy default
        stream).  Every device-pointer call does this by itself while the policy is "torch"."""
        ptr = _torch_stream_ptr(self.device)
        if ptr != self._bound_ptr:
            self._chk(self.lib.qt_set_stream(self._h, ctypes.c_void_p(ptr if ptr else _capi.QT_STREAM_LEGACY)))
            self._bound_ptr = ptr

    def _dev_call(self):
        # binding once was a silent race for a caller that switches torch streams between calls (the handle
        # kept enqueueing on the old stream, unordered with the producers of its inputs).  One raw-pointer read per call.
        if self._stream_policy == "torch":
            self.bind_torch_stream()

    def set_option(self, option, value):
        """qt_set_option: _capi.QT_OPT_SHOTS_CHECK (0 / 1), _capi.QT_OPT_MLE_FUSED_MAX_WAVES (0 = always the split,
        two-loop BFGS path), _capi.QT_OPT_PAIRED_STAGES (0 = the dense-table contraction stages for every one-qubit
        table, 1 = the zero-skipping stages where `paired_tables` says so; the same bits either way),
        _capi.QT_OPT_MLE_SPECIALISE (0 = the generic MLE kernels for every POVM, 1 = the instantiation compiled for the
        six-projector shape where the POVM has it, see `mle_specialised`; the same bits either way),
        _capi.QT_OPT_LIFP_DIST_SLICE (processes per slice of `lifp_dist`; 0 = the library's 128 MB bound),
        _capi.QT_OPT_MLE_HELPER_WAVE (n = 3, one-launch `mle` / `mle_dist` from the 'lin' start: 1 = a helper wavefront
        per trial clips the linear-inversion matrix on speculation beside the first Cholesky sweep and factorises the
        result beside the first evaluation, 0 = the kernel without helpers, see `mle_helper_wave`; the same bits either
        way), _capi.QT_OPT_MHMC_PROCESS_SLICE (n = 3: chains per slice of `mhmc_process_hits`; 0 = the library's 1024; the
        same bits whatever the slice)."""
        self._chk(self.lib.qt_set_option(self._h, int(option), float(value)))

    @property
    def paired_tables(self):
        """Bit 0: the one-qubit table of the current product POVM is paired (six rows, rows 2a and 2a+1 exactly zero
        outside columns 0 and a+1); bit 1: so is its pseudo-inverse as the device computed it.  0 at n >= 4."""
        return self._chk(self.lib.qt_get_paired_tables(self._h))

    @property
    def mle_specialised(self):
        """True if the last `mle` / `mle_dist` launch took the MLE kernels specialised on the POVM's shape (n <= 3:
        'proj-set' with equal shots per setting, paired stages and the shots check on), False if the generic ones."""
        return bool(self._chk(self.lib.qt_get_mle_specialised(self._h)))

    @property
    def mle_helper_wave(self):
        """True if the last `mle` / `mle_dist` launch was the one-launch kernel with a helper wavefront per trial."""
        return bool(self._chk(self.lib.qt_get_mle_helper_wave(self._h)))

    def timer_begin(self):
        self._chk(self.lib.qt_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_double()
        self._chk(self.lib.qt_timer_end(self._h, ctypes.byref(ms)))
        return ms.value

    def timer_stop(self):
        """Record the end event without waiting for it (HIP events on the engine's stream)."""
        self._chk(self.lib.qt_timer_stop(self._h))

    def timer_elapsed(self):
        """Milliseconds between timer_begin() and timer_stop(); waits for the end event."""
        ms = ctypes.c_double(0.0)
        self._chk(self.lib.qt_timer_elapsed(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- a1 / a2 ----------------------------------------------------------------------------
    def pauli_basis(self):
        out = np.empty((self.D, self.d, self.d), dtype=np.complex128)
        self._chk(self.lib.qt_pauli_basis(self._h, _ptr(out), _capi.QT_HOST_PTR))
        return out

    def povm_kron(self, table):
        """table (S1, K1, 4) -> (S1^n, K1^n, 4^n)"""
        table = _f64(table)
        if table.ndim == 2:
            table = table[None]
        s1, k1, four = table.shape
        assert four == 4
        out = np.empty((s1**self.n, k1**self.n, self.D))
        self._chk(self.lib.qt_povm_kron(self._h, _ptr(table), s1, k1, _ptr(out), _capi.QT_HOST_PTR))
        return out

    def povm_kron_dev(self, table, out):
        """device-pointer form: table (S1, K1, 4) float64, out (S1^n, K1^n, 4^n) float64 torch CUDA tensors"""
        self._dev_call()
        s1, k1 = (1, table.shape[0]) if table.dim() == 2 else table.shape[:2]
        assert out.numel() == (s1 * k1 * 4) ** self.n
        self._chk(self.lib.qt_povm_kron(self._h, _ptr(table), s1, k1, _ptr(out), _capi.QT_DEVICE_PTR))

    # ---- a5 ---------------------------------------------------------------------------------
    def set_povm(self, povm_matrix, n_meas):
        """Cache A (S, K, D), the shot weights and the left inverse.  Re-uploading the same
        (povm, shots) pair is skipped.  A tensor that carries its one-qubit factor
        (measurements.PovmTensor) is registered in factorised form (qt_set_povm_product)."""
        factor = povm_matrix.valid_factor() if hasattr(povm_matrix, "valid_factor") else None
        a = _f64(np.asarray(povm_matrix))
        if a.ndim == 2:
            a = a[None]
        s, k, dd = a.shape
        if dd != self.D:
            raise ValueError("Incorrect POVM matrix")
        ns = _f64(np.broadcast_to(np.asarray(n_meas, dtype=np.float64), (s,)))
        # a tensor that still is the tensor power of its factor (checksum just verified) is identified by that
        # factor; only plain arrays are compared byte by byte (64 MB at n = 5: 15 ms per call otherwise)
        key = ((a.shape, povm_matrix.digest(), ns.tobytes(), factor.tobytes()) if factor is not None
               else (a.shape, a.tobytes(), ns.tobytes(), None))
        if key == self._povm_key:
            return
        self._povm_key = None
        self._proc_key = None  # the C side drops its process set-up with the POVM (alloc_povm: proc_set = false)
        if factor is not None and (factor.shape[0] ** self.n, factor.shape[1] ** self.n) == (s, k):
            self._chk(self.lib.qt_set_povm_product(self._h, _ptr(factor), factor.shape[0], factor.shape[1], _ptr(ns),
                                                   _capi.QT_HOST_PTR))
            self.product = True
        else:
            self._chk(self.lib.qt_set_povm(self._h, _ptr(a), s, k, _ptr(ns), _capi.QT_HOST_PTR))
            self.product = False
        self._povm_key = key
        self.S, self.K, self.M = s, k, s * k

    def left_inverse(self):
        out = np.empty((self.D, self.M))
        self._chk(self.lib.qt_get_left_inverse(self._h, _ptr(out), _capi.QT_HOST_PTR))
        return out

    def left_inverse_of(self, a):
        """inv(A^T A) A^T (plain transpose) of an arbitrary real or complex matrix."""
        a = np.asarray(a)
        cplx = np.iscomplexobj(a)
        a = _c128(a) if cplx else _f64(a)
        rows, cols = a.shape
        out = np.empty((cols, rows), dtype=a.dtype)
        self._chk(self.lib.qt_left_inverse(self._h, _ptr(a), rows, cols, int(cplx), _ptr(out), _capi.QT_HOST_PTR))
        return out

    # ---- a11 - a15: process tomography ---------------------------------------------------------
    def process_setup(self, in_states):
        """in_states (D, d, d) complex: design matrix + left inverse for the POVM of `set_povm`."""
        s = _c128(in_states)
        assert s.shape == (self.D, self.d, self.d)
        key = (self._povm_key, s.tobytes())
        if key == self._proc_key:
            return
        self._proc_key = None
        self._chk(self.lib.qt_process_setup(self._h, _ptr(s), _capi.QT_HOST_PTR))
        self._proc_key = key

    def process_operators(self):
        rows, cols = self.D * self.M, self.D * self.D
        oper = np.empty((rows, cols), dtype=np.complex128)
        inv = np.empty((cols, rows), dtype=np.complex128)
        self._chk(self.lib.qt_process_get_operators(self._h, _ptr(oper), _ptr(inv), _capi.QT_HOST_PTR))
        return oper, inv

    def process_prefer_dense(self, on=True):
        """n = 2 keeps the dense left inverse AND its Kronecker factors; `lifp` multiplies by the factors unless this is
        switched on (A/B measurements, tests of the dense-operator kernels)."""
        self._chk(self.lib.qt_process_prefer_dense(self._h, int(bool(on))))

    def process_factors(self):
        """(V_S^+ (D, D), V_P^+ (D, M)): the Kronecker factors of the left inverse (n = 3; n = 2 when M % 4 == 0)."""
        vs = np.empty((self.D, self.D), dtype=np.complex128)
        vp = np.empty((self.D, self.M), dtype=np.complex128)
        self._chk(self.lib.qt_process_get_factors(self._h, _ptr(vs), _ptr(vp), _capi.QT_HOST_PTR))
        return vs, vp

    def lifp(self, counts, cptp=True, return_iters=False):
        """counts (B, D, S, K) or (D, S, K) -> Choi (B, D, D) / (D, D)."""
        c = _i64(counts)
        single = c.ndim == 3
        c = c.reshape(-1, self.D, self.S, self.K)
        b = c.shape[0]
        choi = np.empty((b, self.D, self.D), dtype=np.complex128)
        iters = np.zeros(b, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_lifp_batch(self._h, _ptr(c), b, int(bool(cptp)), _ptr(choi), _ptr(iters), _ptr(status),
                                         _capi.QT_HOST_PTR))
        if single:
            choi, iters = choi[0], iters[0]
        return (choi, iters) if return_iters else choi

    def pgdb(self, counts, n_iter=1000, tol=1e-10, stop="reference", return_iters=False, return_status=False):
        """'pgdb' of process.py:291-308 on counts (B, D, S, K) or (D, S, K) -> Choi.  stop='reference'
        keeps the reference's loop exit (it returns the point before the first improving step),
        stop='converged' accepts steps until the NLL decrease falls below `tol`.  return_iters / return_status append
        the per-trial iteration counts / status codes (_capi.TRIAL_*), in that order."""
        if stop not in ("reference", "converged"):
            raise ValueError("stop must be 'reference' or 'converged'")
        c = _i64(counts)
        single = c.ndim == 3
        c = c.reshape(-1, self.D, self.S, self.K)
        b = c.shape[0]
        choi = np.empty((b, self.D, self.D), dtype=np.complex128)
        iters = np.zeros(b, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_pgdb_batch(self._h, _ptr(c), b, int(n_iter), float(tol), 0 if stop == "reference" else 1,
                                         _ptr(choi), _ptr(iters), _ptr(status), _capi.QT_HOST_PTR))
        if single:
            choi, iters, status = choi[0], iters[0], status[0]
        res = (choi,) + ((iters,) if return_iters else ()) + ((status,) if return_status else ())
        return res[0] if len(res) == 1 else res

    def pgdb_pieces(self, counts, choi):
        """One 'pgdb' iteration's pieces at `choi` (n = 3, qt_pgdb_pieces): counts (D, S, K) and choi (D, D) ->
        (probas (D*M,), grad (D, D) laid out like the Choi matrix, P_CPTP(choi - grad / mu) (D, D)); counts
        (B, D, S, K) and choi (B, D, D) -> the same with a leading B."""
        c = _i64(counts)
        single = c.ndim == 3
        c = c.reshape(-1, self.D, self.S, self.K)
        b = c.shape[0]
        x = _c128(choi).reshape(b, self.D, self.D)
        probas = np.empty((b, c[0].size))
        grad = np.empty((b, self.D, self.D), dtype=np.complex128)
        proj = np.empty((b, self.D, self.D), dtype=np.complex128)
        self._chk(self.lib.qt_pgdb_pieces(self._h, _ptr(c), b, _ptr(x), _ptr(probas), _ptr(grad), _ptr(proj), _capi.QT_HOST_PTR))
        return (probas[0], grad[0], proj[0]) if single else (probas, grad, proj)

    def mhmc_process(self, counts, choi_init, deltas, uniforms, step):
        """Metropolis-Hastings chain(s) of MHMCProcessInterval: counts (D, S, K) or (C, D, S, K), choi_init (D, D) /
        (C, D, D), deltas (T, D*D) / (C, T, D*D) real (column-stacked index), uniforms (T,) / (C, T) ->
        (chain (.., T, D, D) complex, accepted (.., T))."""
        c = _i64(counts)
        single = c.ndim == 3
        c = c.reshape(-1, self.D, self.S, self.K)
        nchain = c.shape[0]
        x0 = _c128(choi_init).reshape(nchain, self.D, self.D)
        dl = _f64(deltas).reshape(nchain, -1, self.D * self.D)
        t = dl.shape[1]
        un = _f64(uniforms).reshape(nchain, t)
        chain = np.empty((nchain, t, self.D, self.D), dtype=np.complex128)
        acc = np.zeros((nchain, t), dtype=np.int32)
        self._chk(self.lib.qt_mhmc_process(self._h, _ptr(c), nchain, _ptr(x0), _ptr(dl), _ptr(un), t, float(step),
                                           _ptr(chain), _ptr(acc), _capi.QT_HOST_PTR))
        return (chain[0], acc[0]) if single else (chain, acc)

    def mhmc_process_draws(self, seed, chains, steps, first_chain=0, first_step=0, out=None):
        """The random numbers of `chains` process chains drawn on the GPU (qt_mhmc_process_draws): (deltas
        (chains, steps, D*D), uniforms (chains, steps)) of global chains first_chain .. and global steps first_step ..,
        each number a function of (seed, chain, step, index) alone (include/qtomo.h states the formula: that of
        `mhmc_draws` with the vector length D*D) -- what `mhmc_process` needs to run the chain of `mhmc_process_hits`.
        NumPy arrays, or `out` = (deltas, uniforms) float64 torch CUDA tensors of those shapes, filled in stream order.
        n <= 2, after `set_povm` and `process_setup`; at n = 3 `mhmc_draws_dim(D * D, ...)` writes the numbers out."""
        chains, steps = int(chains), int(steps)
        ne = self.D * self.D
        if out is not None:
            self._dev_call()
            deltas, uniforms = out
            assert deltas.numel() == chains * steps * ne and uniforms.numel() == chains * steps
            flags = _capi.QT_DEVICE_PTR
        else:
            deltas, uniforms = np.empty((chains, steps, ne)), np.empty((chains, steps))
            flags = _capi.QT_HOST_PTR
        self._chk(self.lib.qt_mhmc_process_draws(self._h, int(seed), int(first_chain), chains, int(first_step), steps,
                                                 _ptr(deltas), _ptr(uniforms), flags))
        return deltas, uniforms

    def mhmc_process_hits(self, counts, centres, choi_init, thresholds, seed, burn_steps, n_points, thinning, step,
                          first_chain=0, return_dist=False, metric=None):
        """One Metropolis-Hastings chain per process with its random numbers drawn on the device and nothing of the
        chain stored (qt_mhmc_process_hits): chain i runs on counts[i] from choi_init[i] with the numbers of global chain
        first_chain + i (`mhmc_process_draws`), `burn_steps` steps and then n_points * thinning of which every
        `thinning`-th state, from the first, is kept.  Returns (hits, accepted): hits[i] = the kept states whose real
        part lies at a Hilbert-Schmidt distance to centres[i] strictly below thresholds[i], accepted[i] = the accepted
        post-burn steps; with return_dist also the kept distances (C, n_points).  counts (C, D, S, K), centres and
        choi_init (C, D, D) complex, thresholds (C,): NumPy arrays (NumPy results) or torch CUDA tensors (tensors, in
        stream order).  metric='trace' / 'if': the same chains with the distance `metric_dist` returns for
        the real part of a kept state and centres[i] (qt_mhmc_process_metric_hits); None: Hilbert-Schmidt.
        n = 3 (qt_mhmc_process_large_hits, qt_mhmc_process_large_metric_hits): the launch family of `mhmc_process` per
        step, drawing the numbers of `mhmc_draws_dim(D * D, ...)`, in slices of QT_OPT_MHMC_PROCESS_SLICE chains.  This
        method is the place that picks the library's entry by the size."""
        code = None if metric is None else self._metric_code(metric)
        return self._chain_hits("qt_mhmc_process" if self.n <= 2 else "qt_mhmc_process_large", code,
                                ((self.D, self.S, self.K), (self.D, self.D), (self.D, self.D)), counts, centres, choi_init,
                                thresholds, seed, burn_steps, n_points, thinning, step, first_chain, return_dist)

    mhmc_process_large_hits = mhmc_process_hits  # (tests and scripts/ call it by this name at n = 3)

    def lifp_dev(self, counts, choi, cptp=True, iters=None, status=None):
        self._dev_call()
        self._chk(self.lib.qt_lifp_batch(self._h, _ptr(counts), counts.shape[0], int(bool(cptp)), _ptr(choi), _ptr(iters),
                                         _ptr(status), _capi.QT_DEVICE_PTR))

    def lifp_dist(self, counts, centre, cptp=True, return_info=False):
        """hs_dst(lifp(counts_b), centre) for every process in ONE pass (qt_lifp_dist_batch: the Choi matrices are not
        written).  counts (B, D, S, K), centre (D, D) -> (B,) float64; return_info appends dict(iters, status).
        A centre table (G, D, D) measures process b against centre[b % G] (qt_lifp_dist_group_batch: the resample-major
        batches of metrics.get_CL_list_channel_boot)."""
        c = _i64(counts).reshape(-1, self.D, self.S, self.K)
        b = c.shape[0]
        cen = _c128(centre)
        assert cen.shape[-2:] == (self.D, self.D) and cen.ndim in (2, 3)
        dist = np.empty(b)
        iters = np.zeros(b, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        if cen.ndim == 3:
            self._chk(self.lib.qt_lifp_dist_group_batch(self._h, _ptr(c), b, int(bool(cptp)), _ptr(cen), cen.shape[0], None,
                                                        _ptr(dist), _ptr(iters), _ptr(status), _capi.QT_HOST_PTR))
        else:
            self._chk(self.lib.qt_lifp_dist_batch(self._h, _ptr(c), b, int(bool(cptp)), _ptr(cen), None, _ptr(dist),
                                                  _ptr(iters), _ptr(status), _capi.QT_HOST_PTR))
        return (dist, dict(iters=iters, status=status)) if return_info else dist

    def lifp_dist_dev(self, counts, centre, dist, cptp=True, choi=None, iters=None, status=None):
        """device-pointer form: counts int64 (B, D, S, K), centre complex128 (D, D), dist float64 (B,) torch CUDA
        tensors; choi complex128 (B, D, D) optional (then what `lifp_dev` writes, bit for bit).  A centre table
        (G, D, D) measures process b against centre[b % G] (qt_lifp_dist_group_batch), as in lin_dist_dev."""
        self._dev_call()
        if centre.dim() == 3:
            self._chk(self.lib.qt_lifp_dist_group_batch(self._h, _ptr(counts), counts.shape[0], int(bool(cptp)), _ptr(centre),
                                                        centre.shape[0], _ptr(choi), _ptr(dist), _ptr(iters), _ptr(status),
                                                        _capi.QT_DEVICE_PTR))
            return
        self._chk(self.lib.qt_lifp_dist_batch(self._h, _ptr(counts), counts.shape[0], int(bool(cptp)), _ptr(centre),
                                              _ptr(choi), _ptr(dist), _ptr(iters), _ptr(status), _capi.QT_DEVICE_PTR))

    def process_born_probs(self, choi, out=None):
        """Outcome probabilities of the channels with Choi matrices `choi` (G, D, D) on the input states of
        `process_setup`: (G, D, S, K) float64, clip(Born(povm, E_g(rho_i)), 0, 1) with E_g the Choi branch of
        Channel.transform (qt_process_born_probs) -- the `pvals` table of the process bootstrap, row (g * D + i) * S + s.
        NumPy in, NumPy out; a complex128 torch CUDA tensor in, `out` (float64 CUDA tensor, allocated when None) out."""
        if _is_dev(choi):
            self._dev_call()
            assert choi.is_contiguous() and tuple(choi.shape[1:]) == (self.D, self.D)
            g = choi.shape[0]
            if out is None:
                import torch

                out = torch.empty((g, self.D, self.S, self.K), dtype=torch.float64, device=choi.device)
            assert out.is_contiguous() and out.numel() == g * self.D * self.M
            self._chk(self.lib.qt_process_born_probs(self._h, _ptr(choi), g, _ptr(out), _capi.QT_DEVICE_PTR))
            return out
        c = _c128(choi).reshape(-1, self.D, self.D)
        p = np.empty((c.shape[0], self.D, self.S, self.K)) if out is None else out
        assert p.dtype == np.float64 and p.flags.c_contiguous and p.size == c.shape[0] * self.D * self.M
        self._chk(self.lib.qt_process_born_probs(self._h, _ptr(c), c.shape[0], _ptr(p), _capi.QT_HOST_PTR))
        return p

    def cptp_project(self, choi, mode="cptp", n_iter=1000, tol=1e-12, return_iters=False):
        """mode 'cptp' (Dykstra) | 'tp' | 'cp' on Choi matrices (B, D, D) / (D, D)."""
        m = {"cptp": 0, "tp": 1, "cp": 2}[mode]
        c = _c128(choi)
        single = c.ndim == 2
        c = c.reshape(-1, self.D, self.D)
        out = np.empty_like(c)
        iters = np.zeros(c.shape[0], dtype=np.int32)
        self._chk(self.lib.qt_cptp_project_batch(self._h, _ptr(c), c.shape[0], m, int(n_iter), float(tol), _ptr(out),
                                                 _ptr(iters), _capi.QT_HOST_PTR))
        if single:
            out, iters = out[0], iters[0]
        return (out, iters) if return_iters else out

    def states_choi(self, states, weights, cptp=True, return_info=False):
        """The 'states' estimator on reconstructed output states (qt_states_choi_batch): states (B, D, d, d) or (D, d, d)
        complex in the order of `process_setup`'s input states, weights (D, D) complex (ProcessTomograph._states_weights)
        -> Choi (B, D, D) / (D, D).  cptp: a trial that fails `is_cptp` is replaced by its `cptp_project`, the others stay
        as assembled; return_info appends dict(projected, iters), per trial."""
        s = _c128(states)
        single = s.ndim == 3
        s = s.reshape(-1, self.D, self.d, self.d)
        w = _c128(weights)
        assert w.shape == (self.D, self.D)
        b = s.shape[0]
        choi = np.empty((b, self.D, self.D), dtype=np.complex128)
        projected = np.zeros(b, dtype=np.int32)
        iters = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_states_choi_batch(self._h, _ptr(s), b, _ptr(w), int(bool(cptp)), _ptr(choi), _ptr(projected),
                                                _ptr(iters), _capi.QT_HOST_PTR))
        if single:
            choi, projected, iters = choi[0], projected[0], iters[0]
        return (choi, dict(projected=projected, iters=iters)) if return_info else choi

    def states_choi_dev(self, states, weights, choi, cptp=True, projected=None, iters=None):
        """device-pointer form: states complex128 (B, D, d, d), weights complex128 (D, D), choi complex128 (B, D, D),
        projected / iters int32 (B,) optional: torch CUDA tensors.  With cptp the call waits for the stream once per slice
        (include/qtomo.h: the number of failing trials sizes the projection)."""
        self._dev_call()
        self._chk(self.lib.qt_states_choi_batch(self._h, _ptr(states), states.shape[0], _ptr(weights), int(bool(cptp)),
                                                _ptr(choi), _ptr(projected), _ptr(iters), _capi.QT_DEVICE_PTR))

    def states_choi_dist_dev(self, states, weights, centres, dist, cptp=True, choi=None, projected=None, iters=None):
        """`states_choi_dev` plus dist[b] = hs_dst(Choi_b, centres[b % G]) for a centre table (G, D, D) -- a single centre
        (D, D) is G = 1 -- into dist float64 (B,) (qt_states_choi_dist_group_batch); choi optional."""
        self._dev_call()
        g = centres.shape[0] if centres.dim() == 3 else 1
        self._chk(self.lib.qt_states_choi_dist_group_batch(self._h, _ptr(states), states.shape[0], _ptr(weights),
                                                           int(bool(cptp)), _ptr(centres), g, _ptr(choi), _ptr(dist),
                                                           _ptr(projected), _ptr(iters), _capi.QT_DEVICE_PTR))

    def is_cptp(self, choi, atol=1e-5):
        """Channel.is_cptp(atol) of Choi matrices (B, D, D) / (D, D) on the device (qt_choi_is_cptp_batch) -> bool array /
        bool.  Equal to the host's answer unless the smallest eigenvalue or the largest trace-preservation residual lies
        within 1e-9 of its threshold.  A torch CUDA tensor in gives an int32 CUDA tensor (1 / 0), in stream order."""
        if _is_dev(choi):
            import torch

            self._dev_call()
            assert choi.is_contiguous() and tuple(choi.shape[1:]) == (self.D, self.D)
            ok = torch.empty(choi.shape[0], dtype=torch.int32, device=choi.device)
            self._chk(self.lib.qt_choi_is_cptp_batch(self._h, _ptr(choi), choi.shape[0], float(atol), _ptr(ok),
                                                     _capi.QT_DEVICE_PTR))
            return ok
        c = _c128(choi)
        single = c.ndim == 2
        c = c.reshape(-1, self.D, self.D)
        ok = np.zeros(c.shape[0], dtype=np.int32)
        self._chk(self.lib.qt_choi_is_cptp_batch(self._h, _ptr(c), c.shape[0], float(atol), _ptr(ok), _capi.QT_HOST_PTR))
        return bool(ok[0]) if single else ok.astype(bool)

    # ---- a4 / a3 ----------------------------------------------------------------------------
    def born_probs(self, bloch, out=None):
        if _is_dev(bloch):
            self._dev_call()
            b = bloch.shape[0]
            self._chk(self.lib.qt_born_probs(self._h, _ptr(bloch), b, _ptr(out), _capi.QT_DEVICE_PTR))
            return out
        bloch = _f64(bloch)
        single = bloch.ndim == 1
        bl = bloch.reshape(-1, self.D)
        p = np.empty((bl.shape[0], self.S, self.K))
        self._chk(self.lib.qt_born_probs(self._h, _ptr(bl), bl.shape[0], _ptr(p), _capi.QT_HOST_PTR))
        return p[0] if single else p

    def bloch_from_matrix(self, mat):
        mat = _c128(mat)
        single = mat.ndim == 2
        m = mat.reshape(-1, self.d, self.d)
        out = np.empty((m.shape[0], self.D))
        self._chk(self.lib.qt_bloch_from_mat(self._h, _ptr(m), m.shape[0], _ptr(out), _capi.QT_HOST_PTR))
        return out[0] if single else out

    def matrix_from_bloch(self, bloch):
        bloch = _f64(bloch)
        single = bloch.ndim == 1
        b = bloch.reshape(-1, self.D)
        out = np.empty((b.shape[0], self.d, self.d), dtype=np.complex128)
        self._chk(self.lib.qt_mat_from_bloch(self._h, _ptr(b), b.shape[0], _ptr(out), _capi.QT_HOST_PTR))
        return out[0] if single else out

    # ---- a6 / a7 ----------------------------------------------------------------------------
    def _counts(self, counts):
        c = _i64(counts)
        single = c.ndim == 2
        c = c.reshape(-1, self.S, self.K) if c.size else c.reshape(0, self.S, self.K)
        return c, single

    def lin(self, counts, physical=True, return_bloch=False):
        c, single = self._counts(counts)
        b = c.shape[0]
        rho = np.empty((b, self.d, self.d), dtype=np.complex128)
        bloch = np.empty((b, self.D)) if return_bloch else None
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_lin_batch(self._h, _ptr(c), b, int(bool(physical)), _ptr(rho), _ptr(bloch), _ptr(status),
                                        _capi.QT_HOST_PTR))
        _check_shots(status)
        if single:
            return (rho[0], bloch[0]) if return_bloch else rho[0]
        return (rho, bloch) if return_bloch else rho

    def lin_dev(self, counts, rho, physical=True, bloch=None, status=None):
        """device-pointer form: counts int64 (B, S, K), rho complex128 (B, d, d) torch CUDA tensors"""
        self._dev_call()
        self._chk(self.lib.qt_lin_batch(self._h, _ptr(counts), counts.shape[0], int(bool(physical)), _ptr(rho),
                                        _ptr(bloch), _ptr(status), _capi.QT_DEVICE_PTR))

    def lin_dist(self, counts, centre, physical=True):
        """hs_dst(point_estimate('lin')(counts_b), centre) for every trial, in ONE pass (qt_lin_dist_batch: the
        estimates themselves are not written).  counts (B, S, K) -> (B,) float64."""
        c, _ = self._counts(counts)
        b = c.shape[0]
        cen = _c128(centre)
        assert cen.shape == (self.d, self.d)
        dist = np.empty(b)
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_lin_dist_batch(self._h, _ptr(c), b, int(bool(physical)), _ptr(cen), None, _ptr(dist),
                                             _ptr(status), _capi.QT_HOST_PTR))
        _check_shots(status)
        return dist

    def lin_dist_dev(self, counts, centre, dist, physical=True, rho=None, status=None):
        """device-pointer form: centre complex128 (d, d), dist float64 (B,) torch CUDA tensors; rho optional.
        A centre table (G, d, d) measures trial b against centre[b % G] (qt_lin_dist_group_batch: resample-major batches
        of the bootstrap coverage study, metrics.get_CL_list_state)."""
        self._dev_call()
        if centre.dim() == 3:
            self._chk(self.lib.qt_lin_dist_group_batch(self._h, _ptr(counts), counts.shape[0], int(bool(physical)),
                                                       _ptr(centre), centre.shape[0], _ptr(rho), _ptr(dist), _ptr(status),
                                                       _capi.QT_DEVICE_PTR))
            return
        self._chk(self.lib.qt_lin_dist_batch(self._h, _ptr(counts), counts.shape[0], int(bool(physical)), _ptr(centre),
                                             _ptr(rho), _ptr(dist), _ptr(status), _capi.QT_DEVICE_PTR))

    # ---- a8 / a9 ----------------------------------------------------------------------------
    def chol_param(self, rho):
        rho = _c128(rho)
        single = rho.ndim == 2
        r = rho.reshape(-1, self.d, self.d)
        x = np.empty((r.shape[0], self.D))
        status = np.zeros(r.shape[0], dtype=np.int32)
        self._chk(self.lib.qt_chol_param(self._h, _ptr(r), r.shape[0], _ptr(x), _ptr(status), _capi.QT_HOST_PTR))
        return (x[0], status[0]) if single else (x, status)

    def chol_unparam(self, x):
        x = _f64(x)
        single = x.ndim == 1
        xx = x.reshape(-1, self.D)
        out = np.empty((xx.shape[0], self.d, self.d), dtype=np.complex128)
        self._chk(self.lib.qt_chol_unparam(self._h, _ptr(xx), xx.shape[0], _ptr(out), _capi.QT_HOST_PTR))
        return out[0] if single else out

    def nll(self, x, counts, grad=True):
        x = _f64(x)
        c, single = self._counts(counts)
        xx = x.reshape(-1, self.D)
        b = xx.shape[0]
        assert c.shape[0] == b
        f = np.empty(b)
        g = np.empty((b, self.D)) if grad else None
        self._chk(self.lib.qt_nll_batch(self._h, _ptr(xx), _ptr(c), b, _ptr(f), _ptr(g), _capi.QT_HOST_PTR))
        if single:
            return (f[0], g[0]) if grad else f[0]
        return (f, g) if grad else f

    # ---- a10 --------------------------------------------------------------------------------
    def mle(self, counts, init="lin", max_iter=100, tol=1e-3, return_info=False):
        if init not in ("lin", "mixed"):
            raise ValueError("Invalid value for argument `init`")
        c, single = self._counts(counts)
        b = c.shape[0]
        rho = np.empty((b, self.d, self.d), dtype=np.complex128)
        nit = np.zeros(b, dtype=np.int32)
        nfev = np.zeros(b, dtype=np.int32)
        fun = np.zeros(b)
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_mle_batch(self._h, _ptr(c), b, _capi.QT_INIT_LIN if init == "lin" else _capi.QT_INIT_MIXED,
                                        int(max_iter), float(tol), _ptr(rho), _ptr(nit), _ptr(nfev), _ptr(fun),
                                        _ptr(status), _capi.QT_HOST_PTR))
        _check_shots(status)
        if single:
            rho, nit, nfev, fun, status = rho[0], nit[0], nfev[0], fun[0], status[0]
        if return_info:
            return rho, dict(nit=nit, nfev=nfev, fun=fun, status=status)
        return rho

    def mhmc_state(self, counts, x_init, deltas, uniforms, step):
        """Metropolis-Hastings chain(s) of mhmc.py on the Cholesky parameters: counts (S, K) or (C, S, K),
        x_init (D,) / (C, D), deltas (T, D) / (C, T, D), uniforms (T,) / (C, T) -> (chain (.., T, D), accepted (.., T)).
        n = 1 .. 5 qubits (k_mhmc_state, n = 4, 5: k_mhmc_state_large, one workgroup per chain)."""
        c, single = self._counts(counts)
        nchain = c.shape[0]
        x0 = _f64(x_init).reshape(nchain, self.D)
        dl = _f64(deltas).reshape(nchain, -1, self.D)
        t = dl.shape[1]
        un = _f64(uniforms).reshape(nchain, t)
        chain = np.empty((nchain, t, self.D))
        acc = np.zeros((nchain, t), dtype=np.int32)
        self._chk(self.lib.qt_mhmc_state(self._h, _ptr(c), nchain, _ptr(x0), _ptr(dl), _ptr(un), t, float(step),
                                         _ptr(chain), _ptr(acc), _capi.QT_HOST_PTR))
        return (chain[0], acc[0]) if single else (chain, acc)

    def mhmc_draws(self, seed, chains, steps, first_chain=0, first_step=0, out=None):
        """The random numbers of `chains` Metropolis-Hastings chains drawn on the GPU (qt_mhmc_draws): (deltas
        (chains, steps, D), uniforms (chains, steps)) of global chains first_chain .. and global steps first_step ..,
        each number a function of (seed, chain, step, index) alone (include/qtomo.h states the formula) -- what
        `mhmc_state` needs to run the chain of `mhmc_state_hits`.  NumPy arrays, or `out` = (deltas, uniforms) float64
        torch CUDA tensors of those shapes, filled in stream order.  n <= 3."""
        chains, steps = int(chains), int(steps)
        if out is not None:
            self._dev_call()
            deltas, uniforms = out
            assert deltas.numel() == chains * steps * self.D and uniforms.numel() == chains * steps
            flags = _capi.QT_DEVICE_PTR
        else:
            deltas, uniforms = np.empty((chains, steps, self.D)), np.empty((chains, steps))
            flags = _capi.QT_HOST_PTR
        self._chk(self.lib.qt_mhmc_draws(self._h, int(seed), int(first_chain), chains, int(first_step), steps, _ptr(deltas),
                                         _ptr(uniforms), flags))
        return deltas, uniforms

    def mhmc_draws_dim(self, dim, seed, chains, steps, first_chain=0, first_step=0, out=None):
        """`mhmc_draws` with the vector length `dim` given (qt_mhmc_draws_dim; even, 2 .. 4096) on an engine of any size:
        (deltas (chains, steps, dim), uniforms (chains, steps)).  dim = D = 256, 1024 feeds `mhmc_state` the numbers of
        `mhmc_state_hits` at n = 4, 5; dim = D at n <= 3 gives the bits of `mhmc_draws`."""
        dim, chains, steps = int(dim), int(chains), int(steps)
        if out is not None:
            self._dev_call()
            deltas, uniforms = out
            assert deltas.numel() == chains * steps * dim and uniforms.numel() == chains * steps
            flags = _capi.QT_DEVICE_PTR
        else:
            deltas, uniforms = np.empty((chains, steps, max(dim, 0))), np.empty((chains, steps))
            flags = _capi.QT_HOST_PTR
        self._chk(self.lib.qt_mhmc_draws_dim(self._h, dim, int(seed), int(first_chain), chains, int(first_step), steps,
                                             _ptr(deltas), _ptr(uniforms), flags))
        return deltas, uniforms

    def mhmc_state_hits(self, counts, centres, x_init, thresholds, seed, burn_steps, n_points, thinning, step, first_chain=0,
                        return_dist=False, metric=None):
        """One Metropolis-Hastings chain per trial with its random numbers drawn on the device and nothing of the chain
        stored (qt_mhmc_state_hits): chain i runs on counts[i] from x_init[i] (`chol_param(centres[i])`) with the numbers
        of global chain first_chain + i (`mhmc_draws`), `burn_steps` steps and then n_points * thinning of which every
        `thinning`-th state, from the first, is kept.  Returns (hits, accepted): hits[i] = the kept states whose
        Hilbert-Schmidt distance to centres[i] lies strictly below thresholds[i], accepted[i] = the accepted post-burn
        steps; with return_dist also the kept distances (C, n_points).  counts (C, S, K), centres (C, d, d) complex,
        x_init (C, D), thresholds (C,): NumPy arrays (NumPy results) or torch CUDA tensors (tensors, in stream order).
        metric='trace' / 'if': the same chains with the distance `metric_dist` returns for a kept state and centres[i]
        (qt_mhmc_state_metric_hits); None: Hilbert-Schmidt.  n = 4, 5 (qt_mhmc_state_large_hits,
        qt_mhmc_state_large_metric_hits): one workgroup per chain drawing the numbers of `mhmc_draws_dim(D, ...)`, the
        steps of `mhmc_state` at these sizes.  This method is the place that picks the library's entry by the size."""
        code = None if metric is None else self._metric_code(metric)
        return self._chain_hits("qt_mhmc_state" if self.n <= 3 else "qt_mhmc_state_large", code,
                                ((self.S, self.K), (self.d, self.d), (self.D,)), counts, centres, x_init, thresholds, seed,
                                burn_steps, n_points, thinning, step, first_chain, return_dist)

    mhmc_state_large_hits = mhmc_state_hits  # (tests and scripts/ call it by this name at n = 4, 5)

    def _chain_hits(self, stem, code, shapes, counts, centres, init, thresholds, seed, burn_steps, n_points, thinning, step,
                    first_chain, return_dist):
        """The argument handling of `mhmc_state_hits` and `mhmc_process_hits`.  code None: the library's `stem`_hits
        (Hilbert-Schmidt); else `stem`_metric_hits, which takes the metric's code behind the handle.  `shapes`: those of
        one chain's counts, of its complex centre and of its starting point (a vector: real; a matrix: complex)."""
        complex_init = len(shapes[2]) == 2
        if _is_dev(counts):
            import torch

            self._dev_call()
            flags = _capi.QT_DEVICE_PTR
            nchain = counts.shape[0]
            args = (counts, centres, init, thresholds)
            assert all(t.is_contiguous() for t in args)
            assert [t.dtype for t in args] == [torch.int64, torch.complex128,
                                               torch.complex128 if complex_init else torch.float64, torch.float64]
            assert [t.numel() for t in args] == [nchain * int(np.prod(s)) for s in shapes] + [nchain]
            hits = torch.zeros(nchain, dtype=torch.int64, device=counts.device)
            acc = torch.zeros(nchain, dtype=torch.int64, device=counts.device)
            dist = torch.empty((nchain, int(n_points)), dtype=torch.float64, device=counts.device) if return_dist else None
        else:
            flags = _capi.QT_HOST_PTR
            counts = _i64(counts).reshape(-1, *shapes[0])
            nchain = counts.shape[0]
            centres = _c128(centres).reshape(nchain, *shapes[1])
            init = (_c128 if complex_init else _f64)(init).reshape(nchain, *shapes[2])
            thresholds = _f64(thresholds).reshape(nchain)
            hits = np.zeros(nchain, dtype=np.int64)
            acc = np.zeros(nchain, dtype=np.int64)
            dist = np.empty((nchain, int(n_points))) if return_dist else None
        tail = (_ptr(counts), nchain, _ptr(centres), _ptr(init), _ptr(thresholds), int(seed), int(first_chain),
                int(burn_steps), int(n_points), int(thinning), float(step), _ptr(hits), _ptr(acc), _ptr(dist), flags)
        if code is None:
            self._chk(getattr(self.lib, stem + "_hits")(self._h, *tail))
        else:
            self._chk(getattr(self.lib, stem + "_metric_hits")(self._h, code, *tail))
        return (hits, acc, dist) if return_dist else (hits, acc)

    def mle_dev(self, counts, rho, init="lin", max_iter=100, tol=1e-3, nit=None, nfev=None, fun=None, status=None):
        self._dev_call()
        self._chk(self.lib.qt_mle_batch(self._h, _ptr(counts), counts.shape[0],
                                        _capi.QT_INIT_LIN if init == "lin" else _capi.QT_INIT_MIXED, int(max_iter),
                                        float(tol), _ptr(rho), _ptr(nit), _ptr(nfev), _ptr(fun), _ptr(status),
                                        _capi.QT_DEVICE_PTR))

    def mle_dist(self, counts, centre, init="lin", max_iter=100, tol=1e-3, return_info=False):
        """hs_dst(point_estimate('mle')(counts_b), centre) for every trial in ONE pass (qt_mle_dist_batch)."""
        if init not in ("lin", "mixed"):
            raise ValueError("Invalid value for argument `init`")
        c, _ = self._counts(counts)
        b = c.shape[0]
        cen = _c128(centre)
        assert cen.shape == (self.d, self.d)
        dist = np.empty(b)
        nit = np.zeros(b, dtype=np.int32)
        status = np.zeros(b, dtype=np.int32)
        self._chk(self.lib.qt_mle_dist_batch(self._h, _ptr(c), b, _capi.QT_INIT_LIN if init == "lin" else _capi.QT_INIT_MIXED,
                                             int(max_iter), float(tol), _ptr(cen), None, _ptr(dist), _ptr(nit), None, None,
                                             _ptr(status), _capi.QT_HOST_PTR))
        _check_shots(status)
        return (dist, dict(nit=nit, status=status)) if return_info else dist

    def mle_dist_dev(self, counts, centre, dist, init="lin", max_iter=100, tol=1e-3, rho=None, nit=None, nfev=None,
                     fun=None, status=None):
        """device-pointer form of mle_dist; a centre table (G, d, d) measures trial b against centre[b % G]
        (qt_mle_dist_group_batch), as in lin_dist_dev"""
        self._dev_call()
        if centre.dim() == 3:
            self._chk(self.lib.qt_mle_dist_group_batch(self._h, _ptr(counts), counts.shape[0],
                                                       _capi.QT_INIT_LIN if init == "lin" else _capi.QT_INIT_MIXED,
                                                       int(max_iter), float(tol), _ptr(centre), centre.shape[0], _ptr(rho),
                                                       _ptr(dist), _ptr(nit), _ptr(nfev), _ptr(fun), _ptr(status),
                                                       _capi.QT_DEVICE_PTR))
            return
        self._chk(self.lib.qt_mle_dist_batch(self._h, _ptr(counts), counts.shape[0],
                                             _capi.QT_INIT_LIN if init == "lin" else _capi.QT_INIT_MIXED, int(max_iter),
                                             float(tol), _ptr(centre), _ptr(rho), _ptr(dist), _ptr(nit), _ptr(nfev),
                                             _ptr(fun), _ptr(status), _capi.QT_DEVICE_PTR))

    # ---- a16 --------------------------------------------------------------------------------
    def hs_dist(self, rho, centre):
        rho = _c128(rho)
        centre = _c128(centre)
        single = rho.ndim == 2
        dim = rho.shape[-1]  # any square size (Choi matrices are 4^n x 4^n), not only this engine's 2^n
        r = rho.reshape(-1, dim, dim)
        assert centre.shape == (dim, dim)
        out = np.empty(r.shape[0])
        self._chk(self.lib.qt_hs_dist_dim(self._h, dim, _ptr(r), _ptr(centre), r.shape[0], _ptr(out), _capi.QT_HOST_PTR))
        return out[0] if single else out

    def device_multinomial(self, n, pvals, rows, seed, first_row=0, out=None):
        """`rows` multinomial draws made on the GPU (qt_device_multinomial): row r ~ multinomial(n[s], pvals[s]),
        s = (first_row + r) % S, from the Philox stream (seed, first_row + r) -- the distribution of
        `np.random.multinomial`, NOT its stream.  n (S,), pvals (S, K) on the host: counts (rows, K) int64 as a NumPy
        array; `out` = an int64 torch CUDA tensor (rows, K): n / pvals may be CUDA tensors too, filled in stream order."""
        if out is not None:
            import torch

            self._dev_call()
            dev = out.device
            n_d = n if _is_dev(n) else torch.as_tensor(np.ascontiguousarray(n, dtype=np.int64)).to(dev)
            p_d = pvals if _is_dev(pvals) else torch.as_tensor(_f64(pvals)).to(dev)
            assert out.dtype == torch.int64 and out.is_contiguous() and out.numel() == rows * p_d.shape[-1]
            self._chk(self.lib.qt_device_multinomial(self._h, seed, first_row, rows, p_d.shape[0], _ptr(n_d), _ptr(p_d),
                                                     p_d.shape[-1], _ptr(out), _capi.QT_DEVICE_PTR))
            self._keep = (n_d, p_d)  # alive until the launch has read them
            return out
        n = np.ascontiguousarray(n, dtype=np.int64)
        pvals = _f64(pvals)
        counts = np.empty((rows, pvals.shape[-1]), dtype=np.int64)
        self._chk(self.lib.qt_device_multinomial(self._h, seed, first_row, rows, pvals.shape[0], _ptr(n), _ptr(pvals),
                                                 pvals.shape[-1], _ptr(counts), _capi.QT_HOST_PTR))
        return counts

    def group_hits(self, dist, thresholds, hits):
        """metrics.py:140-144 for a chunk of whole resamples: hits[g] += #{ r : thresholds[g] > dist[r, g] } (qt_group_hits,
        strict comparison: a NaN distance never counts).  dist float64 (R * G,), thresholds float64 (G,), hits int64 (G,):
        torch CUDA tensors, or NumPy arrays (`hits` is then updated in place too).  `hits` accumulates over calls."""
        if _is_dev(dist):
            self._dev_call()
            flags = _capi.QT_DEVICE_PTR
            assert thresholds.is_contiguous() and hits.is_contiguous() and dist.is_contiguous()
            b, g = dist.numel(), hits.numel()
        else:
            flags = _capi.QT_HOST_PTR
            dist, thresholds = _f64(dist), _f64(thresholds)
            assert isinstance(hits, np.ndarray) and hits.dtype == np.int64 and hits.flags.c_contiguous
            b, g = dist.size, hits.size
        self._chk(self.lib.qt_group_hits(self._h, _ptr(dist), b, g, _ptr(thresholds), _ptr(hits), flags))
        return hits

    def hs_dist_dev(self, rho, centre, out):
        self._dev_call()
        self._chk(self.lib.qt_hs_dist_dim(self._h, rho.shape[-1], _ptr(rho), _ptr(centre), rho.shape[0], _ptr(out),
                                          _capi.QT_DEVICE_PTR))

    _METRICS = {"trace": _capi.QT_METRIC_TRACE, "if": _capi.QT_METRIC_INFIDELITY}

    def _metric_code(self, metric):
        if metric not in self._METRICS:
            raise ValueError(f"metric must be 'trace' or 'if', not {metric!r}")
        return self._METRICS[metric]

    def distance(self, mats, centre, metric=None, g0=0):
        """The distance of every matrix of `mats` to `centre`, whatever their size and this engine's: metric None / 'hs' is
        `hs_dist` (one centre), 'trace' / 'if' is `metric_dist` (a centre, or a table read from row g0).  The package
        measures matrices against a centre through this method and asks about their dimension nowhere else."""
        if metric is None or metric == "hs":
            return self.hs_dist(mats, centre)
        return self.metric_dist(mats, centre, metric, g0)

    def distance_dev(self, mats, centre, dist, metric=None, g0=0):
        """device-pointer form of `distance`: `hs_dist_dev` or `metric_dist_dev` into dist float64 (B,)"""
        if metric is None or metric == "hs":
            return self.hs_dist_dev(mats, centre, dist)
        return self.metric_dist_dev(mats, centre, dist, metric, g0)

    def metric_dist(self, rho, centre, metric, g0=0):
        """Trace distance (metric='trace', geometry.py:23-38) or infidelity ('if', geometry.py:41-56) of Hermitian
        dim x dim matrices to `centre`, whatever this engine's n_qubits, dim = rho.shape[-1] in (2, 4, 8, 16, 32, 64)
        (qt_metric_dist_mat; needs no POVM): states of up to five qubits, the Choi matrix of a channel of up to three.  rho
        (B, dim, dim) or (dim, dim); centre (dim, dim), or a table (G, dim, dim): trial b is then measured against
        centre[(g0 + b) % G].  -> (B,) float64, or a float for a single matrix."""
        code = self._metric_code(metric)
        rho, cen = _c128(rho), _c128(centre)
        single = rho.ndim == 2
        dim = rho.shape[-1]
        r = rho.reshape(-1, dim, dim)
        assert cen.shape[-2:] == (dim, dim) and cen.ndim in (2, 3)
        out = np.empty(r.shape[0])
        self._chk(self.lib.qt_metric_dist_mat(self._h, code, dim, _ptr(r), r.shape[0], _ptr(cen),
                                              cen.shape[0] if cen.ndim == 3 else 1, int(g0), _ptr(out), _capi.QT_HOST_PTR))
        return out[0] if single else out

    def metric_dist_dev(self, rho, centre, dist, metric, g0=0):
        """device-pointer form, dim in (2, 4, 8, 16, 32, 64): rho complex128 (B, dim, dim), centre complex128 (dim, dim) or
        (G, dim, dim), dist float64 (B,) torch CUDA tensors"""
        code = self._metric_code(metric)
        self._dev_call()
        self._chk(self.lib.qt_metric_dist_mat(self._h, code, rho.shape[-1], _ptr(rho), rho.shape[0], _ptr(centre),
                                              centre.shape[0] if centre.dim() == 3 else 1, int(g0), _ptr(dist),
                                              _capi.QT_DEVICE_PTR))

    metric_dist_dim, metric_dist_dim_dev = metric_dist, metric_dist_dev  # (tests and scripts/ call them by these names)

    def sort_quantiles(self, dist, conf_levels):
        """interval.py:610-612 on the device: sort `dist` (NumPy array: a sorted copy is returned; torch CUDA
        tensor: sorted in place) and evaluate interp1d(linspace(0, 1, n), dist) at `conf_levels` -> NumPy array."""
        cl = _f64(np.atleast_1d(conf_levels))
        if cl.size and (cl.min() < 0 or cl.max() > 1):
            raise ValueError("A value in x_new is outside the interpolation range.")
        if _is_dev(dist):
            import torch

            self._dev_call()
            n = dist.numel()
            q = torch.from_numpy(cl).to(dist.device)
            out = torch.empty(cl.size, dtype=torch.float64, device=dist.device)
            self._chk(self.lib.qt_sort_f64(self._h, _ptr(dist), n, _capi.QT_DEVICE_PTR))
            self._chk(self.lib.qt_sorted_quantiles(self._h, _ptr(dist), n, _ptr(q), cl.size, _ptr(out), _capi.QT_DEVICE_PTR))
            self.sync()
            return out.cpu().numpy()
        srt = _f64(dist).copy()
        out = np.empty(cl.size)
        self._chk(self.lib.qt_sort_f64(self._h, _ptr(srt), srt.size, _capi.QT_HOST_PTR))
        self._chk(self.lib.qt_sorted_quantiles(self._h, _ptr(srt), srt.size, _ptr(cl), cl.size, _ptr(out), _capi.QT_HOST_PTR))
        return srt, out


    # ---- f2: stats.py:21-47 ------------------------------------------------------------------------
    def moments(self, counts, n_meas, inv_matrix):
        """Mean and variance of the squared weighted l2 error of the frequencies under multinomial noise
        (reference stats.py l2_mean / l2_variance with the weights of interval.py:88).
        counts (B, S, K) or (S, K); n_meas (S,) shots per setting; inv_matrix (rows, S*K) = left inverse of the design
        matrix / dim.  -> (mean, var), each (B,) or scalars.  Integer-valued counts go to qt_moment_batch; real-valued
        ones (the reference takes any `results`, e.g. expected counts N p) to qt_moment_freq_batch as the frequencies
        counts / n_meas[:, None] (interval.py:82)."""
        c = np.asarray(counts)
        if not (np.issubdtype(c.dtype, np.integer) or np.all(np.equal(np.mod(c, 1), 0))):
            ns = np.broadcast_to(np.asarray(n_meas, dtype=np.float64), (c.shape[-2],))
            return self.moments_freq(c / ns[:, None], ns[0], inv_matrix)
        c = _i64(c)
        single = c.ndim == 2
        if single:
            c = c[None]
        b, s, k = c.shape
        ns = _f64(np.broadcast_to(np.asarray(n_meas, dtype=np.float64), (s,)))
        p = _f64(np.asarray(inv_matrix).reshape(np.asarray(inv_matrix).shape[0], -1))
        assert p.shape[1] == s * k
        mean, var = np.empty(b), np.empty(b)
        self._chk(self.lib.qt_moment_batch(self._h, _ptr(c), b, s, k, _ptr(ns), _ptr(p), p.shape[0], float(ns[0]), _ptr(mean),
                                           _ptr(var), _capi.QT_HOST_PTR))
        return (mean[0], var[0]) if single else (mean, var)

    def moments_freq(self, freq, n_trials, inv_matrix):
        """`moments` from frequencies given directly (qt_moment_freq_batch): freq (B, S, K) or (S, K), n_trials the shots
        per setting of the closing formula (interval.py:89: n_measurements[0])."""
        f = _f64(freq)
        single = f.ndim == 2
        if single:
            f = f[None]
        b, s, k = f.shape
        p = _f64(np.asarray(inv_matrix).reshape(np.asarray(inv_matrix).shape[0], -1))
        assert p.shape[1] == s * k
        mean, var = np.empty(b), np.empty(b)
        self._chk(self.lib.qt_moment_freq_batch(self._h, _ptr(f), b, s, k, _ptr(p), p.shape[0], float(n_trials), _ptr(mean),
                                                _ptr(var), _capi.QT_HOST_PTR))
        return (mean[0], var[0]) if single else (mean, var)

    # ---- f3: interval.py:268-335 -----------------------------------------------------------------------
    def lp_ineq_batch(self, A, C, b, return_x=False):
        """min C[o] . x subject to A x <= b[r] for every r, o (qt_lp_ineq_batch): A (M, N), C (O, N), b (R, M) ->
        (obj (R, O), status (R, O), iters (R, O)[, x (R, O, N)]).  status: _capi.LP_* (obj +inf when infeasible, -inf
        when unbounded, NaN when not converged).  N <= 64."""
        return self._lp_call(self.lib.qt_lp_ineq_batch, A, C, b, return_x)

    def lp_ineq_large_batch(self, A, C, b, return_x=False):
        """lp_ineq_batch for 1 <= N <= 255 variables (qt_lp_ineq_large_batch): the same arguments and results.  The
        normal matrix lives in global memory, the sums run in another order and a vanishing Cholesky pivot is replaced
        instead of ending the program, so at N <= 64 the two agree to the solver's tolerance, not bit for bit."""
        return self._lp_call(self.lib.qt_lp_ineq_large_batch, A, C, b, return_x)

    def lp_ineq_xl_batch(self, A, C, b, return_x=False):
        """lp_ineq_large_batch for 1 <= N <= 1023 variables (qt_lp_ineq_xl_batch): the same arguments and results.
        The normal matrix (8 MB) is formed on the FP64 matrix cores; a workgroup occupies a compute unit, so a call
        runs at most 256 programs at a time and callers split long batches (polytopes.fidelity).  At N <= 255 the two
        agree to the solver's tolerance, not bit for bit."""
        return self._lp_call(self.lib.qt_lp_ineq_xl_batch, A, C, b, return_x)

    def _lp_ineq_by_size(self, A, C, b, return_x=False):
        """The LP kernel for this number of variables -> (lp_ineq_batch's tuple, resolved).  N <= 64 keeps
        lp_ineq_batch and its bits; a right-hand side with a program that it leaves NOT_CONVERGED (its plain Cholesky
        breaks down near a degenerate optimum, e.g. the polytope programs of a pure target state) is solved again by
        lp_ineq_large_batch, whose factorisation replaces a vanishing pivot, and takes that kernel's results for all
        its objectives.  resolved (R,) bool marks those right-hand sides (all True above 64 variables: the large
        kernel solved everything, or above 255 variables lp_ineq_xl_batch, which has the same factorisation)."""
        rhs = _f64(np.atleast_2d(b))
        if np.shape(A)[1] > 255:
            return self.lp_ineq_xl_batch(A, C, rhs, return_x), np.ones(rhs.shape[0], dtype=bool)
        if np.shape(A)[1] > 64:
            return self.lp_ineq_large_batch(A, C, rhs, return_x), np.ones(rhs.shape[0], dtype=bool)
        res = self.lp_ineq_batch(A, C, rhs, return_x)
        resolved = (res[1] == _capi.LP_NOT_CONVERGED).any(axis=1)
        if resolved.any():
            for old, new in zip(res, self.lp_ineq_large_batch(A, C, rhs[resolved], return_x)):
                old[resolved] = new
        return res, resolved

    def lp_pieces(self, kernel, A, w, vm, vn, p1=False, mode=0):
        """The primitives of one LP kernel, run once (qt_lp_pieces; for tests and diagnosis): kernel 0 / 1 / 2 =
        lp_ineq_batch's / lp_ineq_large_batch's / lp_ineq_xl_batch's, A (M, N), weights w (M,), vm (M,), vn (n,) with
        n = N + p1; mode 0 = the kernel's factorisation inside a solve, 1 = its rank test (no border) -> a dict with
        normal (n, n) = A^T diag(w) A, bordered with p1, and factor (n, n) = its Cholesky factor (lower triangles; the
        upper ones keep the entry's 0xFF fill), u (n,) = A^T vm [, sum vm], ax (M,) = A vn[:N], solved (n,) =
        (L L^T)^-1 vn (the fill where ok is 0) and ok (int)."""
        a = _f64(A)
        m, nv = a.shape
        n = nv + (1 if p1 else 0)
        w, vm, vn = _f64(w), _f64(vm), _f64(vn)
        assert w.shape == (m,) and vm.shape == (m,) and vn.shape == (n,)
        out = {"normal": np.empty((n, n)), "factor": np.empty((n, n)), "u": np.empty(n), "ax": np.empty(m),
               "solved": np.empty(n)}
        ok = np.empty(1, dtype=np.int32)
        self._chk(self.lib.qt_lp_pieces(self._h, int(kernel), _ptr(a), m, nv, _ptr(w), _ptr(vm), _ptr(vn), int(bool(p1)), int(mode),
                                        _ptr(out["normal"]), _ptr(out["factor"]), _ptr(out["u"]), _ptr(out["ax"]),
                                        _ptr(out["solved"]), _ptr(ok), _capi.QT_HOST_PTR))
        out["ok"] = int(ok[0])
        return out

    def _lp_call(self, fn, A, C, b, return_x):
        a = _f64(A)
        c = _f64(np.atleast_2d(C))
        rhs = _f64(np.atleast_2d(b))
        m, n = a.shape
        o, r = c.shape[0], rhs.shape[0]
        assert c.shape[1] == n and rhs.shape[1] == m
        obj = np.empty((r, o))
        status = np.empty((r, o), dtype=np.int32)
        iters = np.empty((r, o), dtype=np.int32)
        x = np.empty((r, o, n)) if return_x else None
        self._chk(fn(self._h, _ptr(a), m, n, _ptr(c), o, _ptr(rhs), r, _ptr(obj), _ptr(x), _ptr(status), _ptr(iters),
                     _capi.QT_HOST_PTR))
        return (obj, status, iters, x) if return_x else (obj, status, iters)

    # ---- f4: polytopes/utils.py, verification.py ---------------------------------------------------------
    @staticmethod
    def _polytope_tables(counts, shots):
        """counts (B, R, K) / (B, D, S, K) (NumPy or an int64 torch CUDA tensor), shots (R,) or (S,) (repeated over the
        leading table axes, as utils.py:11 broadcasts them) -> (counts, B, R, K, shots (R,) float64 on the host)."""
        if not _is_dev(counts):
            counts = _i64(counts)
        if counts.ndim < 3:
            raise ValueError("counts must be (trials, settings, outcomes) or (trials, inputs, settings, outcomes)")
        b, k = int(counts.shape[0]), int(counts.shape[-1])
        r = 1
        for s in counts.shape[1:-1]:
            r *= int(s)
        shots = _f64(np.atleast_1d(shots))
        if shots.ndim != 1 or shots.size == 0 or r % shots.size:
            raise ValueError("one shot number per setting")
        return counts, b, r, k, _f64(np.tile(shots, r // shots.size))

    def polytope_confidence(self, counts, shots, deltas):
        """count_confidence (reference polytopes/utils.py:4-13) of every trial at every widening
        (qt_polytope_confidence): counts (B, R, K) or (B, D, S, K), shots (R,) or (S,), deltas (B, Q) or (Q,) (the same
        for every trial) -> conf (B, Q)."""
        c, b, r, k, n = self._polytope_tables(counts, shots)
        if _is_dev(c):
            raise TypeError("polytope_confidence takes NumPy arrays")
        d = _f64(deltas)
        if d.ndim == 1:
            d = _f64(np.broadcast_to(d, (b, d.size)))
        assert d.ndim == 2 and d.shape[0] == b
        conf = np.empty(d.shape)
        self._chk(self.lib.qt_polytope_confidence(self._h, _ptr(c), b, r, k, _ptr(n), _ptr(d), d.shape[1], _ptr(conf),
                                                  _capi.QT_HOST_PTR))
        return conf

    def polytope_coverage(self, counts, shots, levels, truth=None, clip_b=True, return_deltas=False, return_hits=False,
                          covered=None):
        """The coverage study of the confidence polytope over a batch of trials (qt_polytope_coverage; reference
        polytopes/verification.py): delta = count_delta(level) per (trial, level) and, with `truth` (R K true outcome
        probabilities), whether the polytope widened by delta holds the truth (clip_b: test_qst's clipped bound; False:
        test_qpt's).  -> covered (L,) int64, the number of covering trials per level (None without truth); then
        deltas (B, L) and hits (B, L) bool where asked for.  `covered`: an int64 array from earlier chunks to add to.
        counts may be an int64 torch CUDA tensor (the device sampler's): the trials then never visit the host."""
        c, b, r, k, n = self._polytope_tables(counts, shots)
        lv = _f64(np.atleast_1d(levels))
        n_lv = lv.size
        if truth is None and (return_hits or covered is not None):
            raise ValueError("hits and covered need the true outcome probabilities")
        return_deltas = return_deltas or truth is None  # without truth the deltas are all there is to return
        t = None if truth is None else _f64(np.ravel(truth))
        if t is not None and t.size != r * k:
            raise ValueError("truth must hold one probability per table entry")
        cov = None
        if t is not None:
            cov = np.zeros(n_lv, dtype=np.int64) if covered is None else np.ascontiguousarray(covered, dtype=np.int64).copy()
            assert cov.shape == (n_lv,)
        if _is_dev(c):
            import torch

            self._dev_call()
            dev = c.device
            assert c.dtype == torch.int64 and c.is_contiguous()
            to = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
            n_d, lv_d, t_d, cov_d = to(n), to(lv), to(t), to(cov)
            dl_d = torch.empty((b, n_lv), dtype=torch.float64, device=dev) if return_deltas else None
            h_d = torch.empty((b, n_lv), dtype=torch.uint8, device=dev) if return_hits else None
            self._chk(self.lib.qt_polytope_coverage(self._h, _ptr(c), b, r, k, _ptr(n_d), _ptr(lv_d), n_lv, _ptr(t_d),
                                                    int(bool(clip_b)), _ptr(dl_d), _ptr(h_d), _ptr(cov_d), _capi.QT_DEVICE_PTR))
            self.sync()
            cov = None if cov_d is None else cov_d.cpu().numpy()
            dl = None if dl_d is None else dl_d.cpu().numpy()
            hits = None if h_d is None else h_d.cpu().numpy()
        else:
            dl = np.empty((b, n_lv)) if return_deltas else None
            hits = np.empty((b, n_lv), dtype=np.uint8) if return_hits else None
            self._chk(self.lib.qt_polytope_coverage(self._h, _ptr(c), b, r, k, _ptr(n), _ptr(lv), n_lv, _ptr(t),
                                                    int(bool(clip_b)), _ptr(dl), _ptr(hits), _ptr(cov), _capi.QT_HOST_PTR))
        if t is None:
            return dl
        res = (cov,)
        if return_deltas:
            res += (dl,)
        if return_hits:
            res += (hits.astype(bool),)
        return res[0] if len(res) == 1 else res

    def sort_dev(self, x):
        """`x.sort()` in place for a float64 torch CUDA tensor (qt_sort_f64; NaN last like np.sort); asynchronous.  The
        result is np.sort's by value, written canonically: -0.0 as +0.0 and every NaN as 0x7ff8000000000000."""
        self._dev_call()
        self._chk(self.lib.qt_sort_f64(self._h, _ptr(x), x.numel(), _capi.QT_DEVICE_PTR))
        return x

    def quantiles_of_sorted(self, srt, conf_levels):
        """interp1d(linspace(0, 1, n), srt)(conf_levels) for an already sorted CUDA tensor -> NumPy array (synchronises)."""
        import torch

        cl = _f64(np.atleast_1d(conf_levels))
        self._dev_call()
        q = torch.from_numpy(cl).to(srt.device)
        out = torch.empty(cl.size, dtype=torch.float64, device=srt.device)
        self._chk(self.lib.qt_sorted_quantiles(self._h, _ptr(srt), srt.numel(), _ptr(q), cl.size, _ptr(out), _capi.QT_DEVICE_PTR))
        self.sync()
        return out.cpu().numpy()

    # ---- a16 over ranks: the four local steps of the distributed selection (quantpy_amd.distributed) -------------
    def select_splitters(self, srt, stride, n_split, out):
        self._dev_call()
        self._chk(self.lib.qt_select_splitters(self._h, _ptr(srt) if srt.numel() else None, srt.numel(), int(stride),
                                               int(n_split), _ptr(out), _capi.QT_DEVICE_PTR))

    def select_bracket(self, splitters, sizes, stride, n_total, levels, lo_key, hi_key):
        """splitters (N, P) float64, sizes (N,) int64, levels (L,) float64, lo_key / hi_key (L,) int64 (bit patterns)"""
        self._dev_call()
        n_ranks, n_split = splitters.shape
        self._chk(self.lib.qt_select_bracket(self._h, _ptr(splitters), n_ranks, n_split, _ptr(sizes), int(stride),
                                             int(n_total), _ptr(levels), levels.numel(), _ptr(lo_key), _ptr(hi_key),
                                             _capi.QT_DEVICE_PTR))

    def select_window(self, srt, lo_key, hi_key, width, window):
        self._dev_call()
        self._chk(self.lib.qt_select_window(self._h, _ptr(srt) if srt.numel() else None, srt.numel(), _ptr(lo_key),
                                            _ptr(hi_key), lo_key.numel(), int(width), _ptr(window), _capi.QT_DEVICE_PTR))

    def select_finish(self, windows, n_total, levels, out, overflow):
        """windows (N, L, 2 + W) float64 -> out (L,); overflow (1,) int32"""
        self._dev_call()
        n_ranks, n_lev, w2 = windows.shape
        self._chk(self.lib.qt_select_finish(self._h, _ptr(windows), n_ranks, n_lev, w2 - 2, int(n_total), _ptr(levels),
                                            _ptr(out), _ptr(overflow), _capi.QT_DEVICE_PTR))

    def merge_sorted(self, runs, lengths, out=None):
        """Merge sorted runs stored back to back (np.sort's order, NaN last).  runs: float64 torch CUDA tensor (then `out`
        likewise, asynchronous) or NumPy array (a new array is returned); lengths: host integers.  Values keep their bits:
        the two zeros compare equal, as do all NaNs whatever their sign, so runs sorted by np.sort merge correctly."""
        ln = np.ascontiguousarray(lengths, dtype=np.int64)
        if _is_dev(runs):
            import torch

            self._dev_call()
            if out is None:
                out = torch.empty_like(runs)
            assert int(ln.sum()) == runs.numel() == out.numel() and out.data_ptr() != runs.data_ptr()
            self._chk(self.lib.qt_merge_sorted(self._h, _ptr(runs), _ptr(ln), ln.size, _ptr(out), _capi.QT_DEVICE_PTR))
            return out
        r = _f64(runs)
        assert int(ln.sum()) == r.size
        res = np.empty_like(r)
        self._chk(self.lib.qt_merge_sorted(self._h, _ptr(r), _ptr(ln), ln.size, _ptr(res), _capi.QT_HOST_PTR))
        return res


_ENGINES = {}


def engine_key(n_qubits, device=None):
    return (int(n_qubits), default_device() if device is None else int(device))


def get_engine(n_qubits, device=None):
    """Process-wide engine cache: one handle per (n_qubits, device); `device=None` = this process's GPU
    (`default_device`), so that the drop-in classes of rank r run on GPU r."""
    key = engine_key(n_qubits, device)
    eng = _ENGINES.get(key)
    if eng is None:
        eng = _ENGINES[key] = Engine(key[0], key[1])
    return eng


def any_engine(device=None):
    """An engine of this process's GPU for work that does not depend on the qubit number (the device sampler, sorting):
    one that exists already, else the one-qubit engine."""
    dev = default_device() if device is None else int(device)
    for (_, d), eng in _ENGINES.items():
        if d == dev:
            return eng
    return get_engine(1, dev)


def status_text(code):
    return _STATUS_TEXT.get(int(code), "ok")
