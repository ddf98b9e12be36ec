/* qtomo.h -- C ABI of libqtomo.so, the MI355X (gfx950) tomography-reconstruction engine.
 *
 * The reference (nordmtr/quantpy) is pure Python and has no FFI; this boundary sits directly
 * beneath the reference methods cited on each entry point (paths are into the reference tree,
 * SURVEY.md section 8a/8b).  INTEGRATION.md shows the ctypes binding a quantpy maintainer would
 * add; quantpy_amd/_capi.py is that binding for this repository's drop-in classes.
 *
 * Conventions
 *   - n qubits, d = 2^n, D = 4^n; a POVM is a tensor A[S][K][D] of Bloch rows (M = S*K rows).
 *   - all arrays are caller-owned and C-contiguous; complex = interleaved double[2] (re, im).
 *   - pointers are HOST pointers unless `flags & QT_DEVICE_PTR`, in which case every array
 *     argument of that call is a device pointer valid on the handle's device and the call is
 *     asynchronous on the handle's stream (qt_sync to wait).
 *   - every function returns 0 on success and a negative qt_status on argument / runtime errors
 *     (qt_last_error() gives the text).  Batched estimators additionally fill a per-trial
 *     `int32 status[B]` with qt_trial_status and, for host-pointer calls, return the number of
 *     trials whose status is non-zero.
 *   - a handle is bound to one device and one stream and is not thread-safe; use one handle per
 *     host thread.  No exception crosses the ABI.  There is no CPU fallback: without a usable
 *     HIP device qt_create fails.
 */
#ifndef QTOMO_H
#define QTOMO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qt_handle qt_handle_t;

enum qt_status {
  QT_OK = 0,
  QT_ERR_ARG = -1,      /* bad argument (null pointer, size, n_qubits out of range) */
  QT_ERR_STATE = -2,    /* call order: e.g. estimator before qt_set_povm */
  QT_ERR_HIP = -3,      /* HIP runtime error */
  QT_ERR_SINGULAR = -4, /* A^T A is singular: the POVM is not informationally complete */
  QT_ERR_UNSUPPORTED = -5
};

enum qt_trial_status {
  QT_TRIAL_OK = 0,
  QT_TRIAL_NOT_PD = 1,      /* Cholesky pivot <= 0: scipy.linalg.cholesky raises LinAlgError   */
  QT_TRIAL_LINESEARCH = 2,  /* both line searches failed: scipy BFGS warnflag 2                 */
  QT_TRIAL_MAXITER = 3,     /* iteration cap reached: scipy BFGS warnflag 1                     */
  QT_TRIAL_NAN = 4,         /* NaN in value, gradient or parameters: scipy BFGS warnflag 3      */
  QT_TRIAL_SHOTS = 5        /* the trial's per-setting totals are not proportional to the Ns registered with
                               qt_set_povm: the reference would weight this trial differently
                               (state.py:138-141, 194-197); the returned estimate is not meaningful  */
};

enum qt_flags { QT_HOST_PTR = 0, QT_DEVICE_PTR = 1 };
enum qt_init { QT_INIT_LIN = 0, QT_INIT_MIXED = 1 };

/* ---- library / handle ------------------------------------------------------------------ */
int qt_version(void);
const char* qt_last_error(void);
/* number of HIP devices visible, or a negative qt_status */
int qt_device_count(void);
/* n_qubits in 1..5.  State estimators: any POVM at every n (n = 4, 5: a product POVM registered with
 * qt_set_povm_product contracts qubit by qubit; a plain tensor takes the streaming dense path).  Process
 * tomography: n <= 3 (n = 3 through the Kronecker factors of the design matrix, see qt_process_setup). */
qt_handle_t* qt_create(int device, int n_qubits);
void qt_destroy(qt_handle_t* h);
int qt_sync(qt_handle_t* h);
/* Run the handle's work on an existing hipStream_t (e.g. torch's current stream); NULL = a private
 * non-blocking stream (the default after qt_create); QT_STREAM_LEGACY = the legacy default ("null")
 * stream, which is what a framework means by stream 0.
 * ORDERING CONTRACT of device-pointer calls (flags & QT_DEVICE_PTR): they are enqueued on the handle's
 * stream and return at once.  Inputs must have been produced on that stream, or by work the caller has
 * already ordered before it (event / synchronize); outputs may be consumed on that stream, after
 * qt_sync, or after the caller's own event on it.  A caller whose producers run on another stream
 * (torch's current stream, say) either binds the handle to that stream with qt_set_stream or orders
 * the two streams itself.  Every call leaves the calling thread's current HIP device unchanged. */
#define QT_STREAM_LEGACY ((void*)1)
int qt_set_stream(qt_handle_t* h, void* hip_stream);
/* Per-handle switches.  QT_OPT_SHOTS_CHECK (default 1): compare every trial's per-setting totals with the Ns of
 * qt_set_povm (QT_TRIAL_SHOTS).  QT_OPT_MLE_FUSED_MAX_WAVES (default 1024): batches of up to this many trial-wavefronts
 * (n <= 3) run the MLE as one launch with the BFGS inverse Hessian in registers; larger ones as a start launch plus a
 * BFGS launch in two-loop form (0 = always the latter).  Both forms compute scipy's iterates.
 * QT_OPT_PAIRED_STAGES (default 1): at n <= 3 a six-row one-qubit table whose rows 2a, 2a+1 are exactly zero outside
 * columns 0 and a+1 ('proj-set', 'proj' and their pseudo-inverses) runs contraction stages that skip those zeros;
 * 0 forces the dense-table stages.  Both give the same bits, the sign of a zero excepted.
 * QT_OPT_MLE_SPECIALISE (default 1): at n <= 3 the MLE kernels have a second instantiation compiled for the shape of
 * every built-in six-projector run ('proj-set': both tables paired and QT_OPT_PAIRED_STAGES on, equal shots per
 * setting, QT_OPT_SHOTS_CHECK on); 0 forces the generic instantiation.  Both give the same bits.
 * QT_OPT_LIFP_DIST_SLICE (default 0): qt_lifp_dist_batch runs its batch in slices of this many processes, so that the
 * workspaces that follow the batch stay bounded; 0, or more than 128 MB of Choi matrices (2048 processes at n = 3,
 * 32 768 at n = 2), takes that bound.  The same bits whatever the slice.
 * QT_OPT_MLE_HELPER_WAVE (default 1): at n = 3 the one-launch MLE from the 'lin' start (product POVM, batches within
 * QT_OPT_MLE_FUSED_MAX_WAVES) gives every trial a twin wavefront, which reads the trial's counts itself, forms the same
 * linear-inversion matrix and lifts it on speculation beside the first Cholesky sweep; where the sweep asks for the
 * lift, the twin keeps the clipped matrix and goes on as the trial (evaluation, outputs, BFGS loop) while the first
 * wavefront factorises that matrix for it.  The launch keeps 16 instead of 24 BFGS pairs per trial in LDS, and where
 * its layout does not fit a CU's LDS the kernel without twins runs; 0 launches that kernel.  Both give the same bits.
 * QT_OPT_MHMC_PROCESS_SLICE (default 0): qt_mhmc_process_large_hits and qt_mhmc_process_large_metric_hits run their
 * chains in slices of this many, which bounds their workspace (about 0.6 MB per chain of a slice); 0 takes 1024.  The
 * same bits whatever the slice. */
enum qt_option {
  QT_OPT_SHOTS_CHECK = 1,
  QT_OPT_MLE_FUSED_MAX_WAVES = 2,
  QT_OPT_PAIRED_STAGES = 3,
  QT_OPT_MLE_SPECIALISE = 4,
  QT_OPT_LIFP_DIST_SLICE = 5,
  QT_OPT_MLE_HELPER_WAVE = 6,
  QT_OPT_MHMC_PROCESS_SLICE = 7
};
int qt_set_option(qt_handle_t* h, int option, double value);
/* Which one-qubit tables of the current product POVM have that shape: bit 0 = T, bit 1 = pinv(T) as computed on the
 * device (0 without a product POVM and at n >= 4; independent of QT_OPT_PAIRED_STAGES). */
int qt_get_paired_tables(qt_handle_t* h);
/* 1 if the last qt_mle_batch / qt_mle_dist_batch launch took the specialised instantiation, else 0. */
int qt_get_mle_specialised(qt_handle_t* h);
/* 1 if the last qt_mle_batch / qt_mle_dist_batch launch was the kernel with helper wavefronts, else 0. */
int qt_get_mle_helper_wave(qt_handle_t* h);
/* hipEvent timers on the handle's stream: begin, ..., end -> elapsed milliseconds */
int qt_timer_begin(qt_handle_t* h);
int qt_timer_end(qt_handle_t* h, double* elapsed_ms);
/* the two halves of qt_timer_end: record the end event (asynchronous) / wait for it and read the interval */
int qt_timer_stop(qt_handle_t* h);
int qt_timer_elapsed(qt_handle_t* h, double* elapsed_ms);

/* ---- a1: quantpy/routines.py:14-19 generate_pauli ---------------------------------------- */
/* out[D][d][d][2]: P_k = P_k1 (x) ... (x) P_kn, k = sum_j k_j 4^(n-1-j) */
int qt_pauli_basis(qt_handle_t* h, double* out, int flags);

/* ---- a2: quantpy/measurements.py:88-93 generate_measurement_matrix (array / string path) - */
/* povm1[S1][K1][4] one-qubit table -> out[S1^n][K1^n][D], all three axes Kronecker'd */
int qt_povm_kron(qt_handle_t* h, const double* povm1, int S1, int K1, double* out, int flags);

/* ---- a5 + cache: quantpy/routines.py:69-71 _left_inv; state.py:194-197, 222-225 ----------- */
/* Stores A[S][K][D], the shot-weighted A' = A * Ns[s] / sum(Ns) reshaped (M, D), and the left
 * inverse inv(A'^T A') A'^T (plain transpose).  Ns[S] = shots per setting (as float64, like the
 * reference's n_measurements).  Every later estimator call on this handle uses this POVM and
 * assumes each trial's per-setting totals equal Ns. */
int qt_set_povm(qt_handle_t* h, const double* A, int S, int K, const double* Ns, int flags);
/* The same for a POVM given as a one-qubit table povm1[S1][K1][4] to be tensored n times
 * (measurements.py:88-93: every built-in POVM and every array whose last axis is 4).  Builds the
 * full tensor on the device and, in addition, keeps the factorised form: the estimators then
 * contract qubit by qubit instead of over the dense M x D operand.  Ns[S1^n]. */
int qt_set_povm_product(qt_handle_t* h, const double* povm1, int S1, int K1, const double* Ns, int flags);
/* out[D][M]: the cached left inverse (for inspection / tests) */
int qt_get_left_inverse(qt_handle_t* h, double* out, int flags);

/* the same left inverse for an arbitrary rows x cols matrix, real (is_complex = 0) or complex
 * (interleaved; still the PLAIN transpose, as routines.py:71 writes it): out[cols][rows] */
int qt_left_inverse(qt_handle_t* h, const double* A, int rows, int cols, int is_complex, double* out, int flags);

/* ---- a4: quantpy/tomography/state.py:109-110 (probabilities only; sampling stays on host) -- */
/* p[B][S][K] = clip(d * sum_k A[s][k'][k] bloch[b][k], 0, 1) */
int qt_born_probs(qt_handle_t* h, const double* bloch, int B, double* p, int flags);

/* ---- a3: quantpy/qobj.py:109-135 + geometry.py:59-70 --------------------------------------- */
/* bloch[b][k] = Re Tr(P_k M_b^dagger) / d ;  M_b = sum_k bloch[b][k] P_k */
int qt_bloch_from_mat(qt_handle_t* h, const double* mat, int B, double* bloch, int flags);
int qt_mat_from_bloch(qt_handle_t* h, const double* bloch, int B, double* mat, int flags);

/* ---- a4 / a12 / a16 host side: state.py:109-114, the draws behind experiment() ----------------- */
/* rows x `np.random.multinomial(n[s], pvals[s])` with s = row % period -- NumPy's legacy sampler (MT19937 doubles,
 * conditional binomials by BTPE / inversion) restated bit for bit on the generator state the caller passes:
 * mt_key[624] and *mt_pos are those of `np.random.get_state()`, advanced in place by exactly the words NumPy
 * would have consumed, so `np.random.set_state()` afterwards leaves the global stream where the reference's
 * loop of Python calls leaves it.  pvals[period][K], out[rows][K].  Host memory only; needs no handle and no
 * GPU.  QT_ERR_ARG (with NumPy's message) when a pvals row fails RandomState.multinomial's own checks. */
int qt_legacy_multinomial(uint32_t* mt_key, int* mt_pos, long long rows, int period, const int64_t* n,
                          const double* pvals, int K, int64_t* out);

/* The same draws for callers that do NOT need the reference's stream (opt-in; state.py:109-114 only fixes the
 * distribution): row r is a multinomial(n[s], pvals[s]), s = (first_row + r) % period, made on the GPU by one thread
 * from its own Philox4x32-10 stream keyed by (seed, first_row + r) through the same conditional BTPE / inversion
 * binomials -- so the table depends on (seed, global row index) only, however the rows are split over calls or ranks,
 * and with QT_DEVICE_PTR the counts never leave HBM on their way to qt_lin/mle_batch.  n[period], pvals[period][K],
 * out[rows][K].  Host-pointer calls check pvals like RandomState.multinomial does (QT_ERR_ARG); device-pointer calls
 * clamp each conditional probability into [0, 1] (a NaN counts as 0). */
int qt_device_multinomial(qt_handle_t* h, uint64_t seed, uint64_t first_row, long long rows, int period,
                          const int64_t* n, const double* pvals, int K, int64_t* out, int flags);
/* The generator block behind it, on the host, for known-answer tests: out[4] = Philox4x32-10(ctr[4], key[2]). */
void qt_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out);

/* ---- a6 + a7: state.py:191-202 _point_estimate_lin, :267-273 _make_feasible ---------------- */
/* counts[B][S][K] int64 -> rho[B][d][d][2].  physical != 0: eigenvalues clipped at 1e-15 and
 * the trace renormalised.  bloch_out (nullable): the linear-inversion Bloch vector [B][D]. */
int qt_lin_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, double* rho, double* bloch_out,
                 int32_t* status, int flags);

/* ---- a6/a7 + a16 in one pass: the body of the bootstrap loop, quantpy/tomography/interval.py:600-609 -------
 * qt_lin_batch plus dist[b] = hs_dst(estimate_b, centre) (geometry.py:5-20, as qt_hs_dist_batch computes it).
 * centre[d][d][2]; rho is NULLABLE here: a bootstrap needs one double per resample, not the matrices. */
int qt_lin_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, const double* centre, double* rho,
                      double* dist, int32_t* status, int flags);

/* ---- a8: quantpy/routines.py:84-101 Cholesky parametrisation ------------------------------- */
/* x[B][D] = [diag L | Re L_(i>j) | Im L_(i>j)] (strict lower in np.tril_indices order) of
 * rho[B][d][d][2] = L L^dagger ; and back (LLh = L L^dagger, not normalised) */
int qt_chol_param(qt_handle_t* h, const double* rho, int B, double* x, int32_t* status, int flags);
int qt_chol_unparam(qt_handle_t* h, const double* x, int B, double* LLh, int flags);

/* ---- a9: state.py:217-229 _nll (value) and its exact gradient ------------------------------ */
/* f[b] = -sum_m freq_m log(d (A' b(x_b))_m + 1e-10), freq = counts / sum(counts);
 * grad (nullable) [B][D] = df/dx (analytic; the reference differentiates numerically) */
int qt_nll_batch(qt_handle_t* h, const double* x, const int64_t* counts, int B, double* f, double* grad, int flags);

/* ---- a10: state.py:204-215 _point_estimate_mle_chol + scipy BFGS --------------------------- */
/* tol is scipy's gtol (inf-norm of the gradient); max_iter its maxiter.  Outputs (each nullable
 * except rho): nit[B] BFGS iterations, nfev[B] value+gradient evaluations (the reference's own
 * nfev, which also counts its finite-difference probes, equals nfev * (D + 1)), fun[B] final
 * objective, status[B]. */
int qt_mle_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol, double* rho,
                 int32_t* nit, int32_t* nfev, double* fun, int32_t* status, int flags);

/* ---- a8-a10 + a16 in one pass (interval.py:600-609 with method='mle'): qt_mle_batch plus the Hilbert-Schmidt
 * distance of every estimate to centre[d][d][2]; rho NULLABLE (8 bytes written per resample instead of 16 d^2). */
int qt_mle_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol,
                      const double* centre, double* rho, double* dist, int32_t* nit, int32_t* nfev, double* fun,
                      int32_t* status, int flags);

/* ---- the bootstrap coverage study, quantpy/metrics.py:125-144 (get_CL_list_state with interval='boot'): every trial t of
 * the study resamples around ITS OWN point estimate, so a batch of resamples has a centre per trial ----------------------
 * qt_lin_dist_batch / qt_mle_dist_batch with a table centres[G][d][d][2]: dist[b] = hs_dst(estimate_b, centres[b % G]).
 * The batch is resample-major, counts[r * G + t] = resample r of trial t -- the order qt_device_multinomial writes with
 * period = G * S and the Born probabilities of the G estimates as pvals.  G >= 1 (else QT_ERR_ARG); G = 1 is
 * qt_lin_dist_batch / qt_mle_dist_batch.  Everything else -- rho NULLABLE, the outputs, status -- as in those. */
int qt_lin_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, const double* centres, int G,
                            double* rho, double* dist, int32_t* status, int flags);
int qt_mle_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol,
                            const double* centres, int G, double* rho, double* dist, int32_t* nit, int32_t* nfev,
                            double* fun, int32_t* status, int flags);
/* metrics.py:140-144, `np.where(delta > distances)` for every trial of a chunk of whole resamples: dist[B] as the two
 * entries above write it (B = R * G, else QT_ERR_ARG), thresholds[G] = delta_t;  hits[g] += #{ r : thresholds[g] >
 * dist[r * G + g] }, int64.  The comparison is strict, so a NaN distance never counts.  `hits` ACCUMULATES (zero it before
 * the first chunk): integer adds, so the totals do not depend on how the resamples are chunked. */
int qt_group_hits(qt_handle_t* h, const double* dist, int B, int G, const double* thresholds, int64_t* hits, int flags);

/* ---- a16: quantpy/geometry.py:5-20 hs_dst --------------------------------------------------- */
/* dist[b] = sqrt(|Tr((rho_b - centre)^2)|) / sqrt(2), set to 0 below 1e-15 */
int qt_hs_dist_batch(qt_handle_t* h, const double* rho, const double* centre, int B, double* dist, int flags);
/* the same for dim x dim matrices whatever the handle's n_qubits (Choi matrices of an n-qubit channel: dim = 4^n) */
int qt_hs_dist_dim(qt_handle_t* h, int dim, const double* rho, const double* centre, int B, double* dist, int flags);

/* ---- quantpy/geometry.py:23-38 trace_dst, :41-56 if_dst, for a batch against a table of centres -------------------
 * dist[b] = metric(rho_b, centres[(g0 + b) % G]); rho[B][d][d][2], centres[G][d][d][2] with d = 2^n the handle's
 * dimension, n <= 3 (n = 4, 5: QT_ERR_UNSUPPORTED); needs no POVM.  G = 1, g0 = 0: one centre.  A table with g0 serves a
 * resample-major batch that starts inside a resample (see qt_lin_dist_group_batch).
 * Both arguments are taken to be HERMITIAN (the imaginary parts of the diagonals are dropped, the strict lower triangle of
 * a matrix that is not Hermitian is not what the reference's sqrtm would see); each value comes from the eigenvalues of
 * one Hermitian matrix per trial, by the Jacobi sweeps of the eigenvalue clip:
 *   QT_METRIC_TRACE       sum_i |lambda_i(rho_b - centre)| / 2        (|Tr sqrtm(Delta Delta)| / 2 for Hermitian Delta)
 *   QT_METRIC_INFIDELITY  1 - (sum_i sqrt(max(mu_i, 0)))^2, mu = eigenvalues of the Hermitian part of S rho_b S with
 *                         S = the Hermitian root of the centre, negative eigenvalues clipped to 0, formed once per call
 *                         and centre (fidelity is symmetric: the reference takes the root of its first argument)
 * A value below 1e-15 -- small negative infidelities included -- is returned as 0, as the reference returns it.  A NaN
 * (or an infinity) in rho_b or in its centre gives dist[b] = NaN and touches no other trial; a trial's bits depend on
 * its two matrices alone, not on B, G, g0 or its place in the batch.
 * QT_ERR_ARG: an unknown metric, G < 1, g0 outside [0, G), B < 0, a null array with B > 0.  B == 0 returns 0. */
enum qt_metric { QT_METRIC_TRACE = 0, QT_METRIC_INFIDELITY = 1 };
int qt_metric_dist_group_batch(qt_handle_t* h, int metric, const double* rho, int B, const double* centres, int G, int g0,
                               double* dist, int flags);
/* ---- the same (quantpy/geometry.py:23-38 trace_dst, :41-56 if_dst) for dim x dim matrices on ANY handle ------------
 * dist[b] = metric(rho_b, centres[(g0 + b) % G]); rho[B][dim][dim][2], centres[G][dim][dim][2], whatever the handle's
 * n_qubits (as qt_hs_dist_dim); needs no POVM.
 *   dim = 2, 4, 8   the kernels of qt_metric_dist_group_batch: the same bits as that entry on a handle of that size
 *   dim = 16, 32    four- and five-qubit states, the Choi matrix of a two-qubit channel: one workgroup per trial, the same
 *                   Jacobi sweeps (at most 32 of them instead of 20) and the same formulas, element for element
 *   any other dim   QT_ERR_UNSUPPORTED (supported: 2, 4, 8, 16, 32; a three-qubit Choi matrix is dim = 64)
 * Both arguments are taken to be HERMITIAN, exactly as above: the imaginary parts of the diagonals are dropped, the trace
 * distance is sum_i |lambda_i(rho_b - centre)| / 2, the infidelity 1 - (sum_i sqrt(max(mu_i, 0)))^2 with mu the
 * eigenvalues of the Hermitian part of S rho_b S, S = the clipped Hermitian root of the centre, formed once per call and
 * centre.  A value below 1e-15 -- small negative infidelities included -- is returned as 0.  A NaN (or an infinity) in
 * rho_b or in its centre gives dist[b] = NaN and touches no other trial; a trial's bits depend on its two matrices
 * alone, not on B, G, g0 or its place in the batch.
 * QT_ERR_ARG: an unknown metric, G < 1, g0 outside [0, G), B < 0, a null array with B > 0.  B == 0 returns 0. */
int qt_metric_dist_dim(qt_handle_t* h, int metric, int dim, const double* rho, int B, const double* centres, int G, int g0,
                       double* dist, int flags);
/* ---- the same (quantpy/geometry.py:23-38 trace_dst, :41-56 if_dst) up to dim = 64, the Choi matrix of a three-qubit
 * channel; a sibling because qt_metric_dist_dim's refusal of dim = 64 is part of that entry's contract -----------------
 * dist[b] = metric(rho_b, centres[(g0 + b) % G]); rho[B][dim][dim][2], centres[G][dim][dim][2], on ANY handle, whatever
 * its n_qubits; needs no POVM.
 *   dim = 2, 4, 8, 16, 32   the code of qt_metric_dist_dim: the same bits as that entry
 *   dim = 64                one workgroup of 1024 threads per trial, four elements per thread; a round's 32 rotations are
 *                           formed once and handed round through LDS; at most 48 sweeps; the same formulas, but NOT the
 *                           bits a one-thread-per-element kernel would give: the values are within 1e-13 max(1, Tr)
 *                           (trace distance) and 1e-12 (infidelity of full-rank arguments; 1e-6 otherwise) of float64
 *                           linear algebra.  135 296 B of LDS per workgroup.
 *   any other dim           QT_ERR_UNSUPPORTED (supported: 2, 4, 8, 16, 32, 64)
 * Both arguments are taken to be HERMITIAN, exactly as above: the imaginary parts of the diagonals are dropped, the trace
 * distance is sum_i |lambda_i(rho_b - centre)| / 2, the infidelity 1 - (sum_i sqrt(max(mu_i, 0)))^2 with mu the
 * eigenvalues of the Hermitian part of S rho_b S, S = the clipped Hermitian root of the centre (the SECOND argument),
 * formed once per call and centre into the handle's workspace (G * 2 * dim^2 doubles).  A value below 1e-15 -- small
 * negative infidelities included -- is returned as +0.  A NaN (or an infinity) in rho_b or in its centre gives
 * dist[b] = NaN and touches no other trial; a trial's bits depend on its two matrices alone, not on B, G, g0, its place in
 * the batch or host- against device-pointer staging.
 * QT_ERR_ARG: an unknown metric, G < 1, g0 outside [0, G), B < 0, a null array with B > 0.  B == 0 returns 0. */
int qt_metric_dist_mat(qt_handle_t* h, int metric, int dim, const double* rho, int B, const double* centres, int G, int g0,
                       double* dist, int flags);

/* ---- a16: quantpy/tomography/interval.py:610-612 (and :683-685) -------------------------------- */
/* `dist.sort()`: ascending in-place sort of n float64 values in np.sort's order (NaN last; bitonic in LDS up to 8192
 * values, device radix sort above).  The output is np.sort's by value, with canonical bits: either zero is written as
 * +0.0 and every NaN, whatever its sign and payload, as the quiet NaN 0x7ff8000000000000. */
int qt_sort_f64(qt_handle_t* h, double* x, long long n, int flags);
/* `interp1d(np.linspace(0, 1, n), sorted)(conf_levels)`: scipy's linear interp1d on real 1-D data is numpy.interp, and
 * these are its semantics on the grid x_i = i / (n - 1) -- cell x_j <= q < x_(j+1), a level ON a grid point returns
 * sorted[j] itself, otherwise slope * (q - x_j) + y_j operation by operation; out[n_levels].  A level outside [0, 1]
 * gives NaN (interp1d raises there). */
int qt_sorted_quantiles(qt_handle_t* h, const double* sorted, long long n, const double* conf_levels, int n_levels,
                        double* out, int flags);

/* ---- a16 when the distances are spread over N ranks (one process per GPU): interval.py:610-612 without gathering
 * the sample.  Every rank sorts ITS shard (qt_sort_f64); interp1d at a confidence level q needs the order statistics
 * k0 = floor-cell(q) and k0 + 1 of the union only.  Four small steps with two all-gathers of a few KB in between
 * (quantpy_amd/distributed.py does those with torch.distributed; the C ABI stays free of collectives):
 *   qt_select_splitters : splitters[j] = sorted[j * stride], j < P (padded behind everything)        -> all-gather [N][P]
 *   qt_select_bracket   : from all ranks' splitters and shard sizes: per level the tightest splitter pair
 *                         (lo, hi] that provably holds both order statistics (as radix-sort keys; 0 / ~0 = none)
 *   qt_select_window    : window[l] = { #values <= lo, w = #values in (lo, hi], the first min(w, W) of them } -> all-gather
 *   qt_select_finish    : out[l] = interp1d(linspace(0, 1, n_total), sorted union)(conf_levels[l]); *overflow != 0 when a
 *                         window was clipped (w > W, heavy ties) or the union exceeds the kernel's capacity: the caller
 *                         then gathers the sorted shards and merges them (qt_merge_sorted) instead.
 * W >= (2 N + 3) * stride covers every sample without massive ties.  Same results as np.sort + interp1d, bit for bit. */
int qt_select_splitters(qt_handle_t* h, const double* sorted, long long n, long long stride, int P, double* splitters,
                        int flags);
int qt_select_bracket(qt_handle_t* h, const double* splitters, int N, int P, const int64_t* sizes, long long stride,
                      long long n_total, const double* conf_levels, int L, uint64_t* lo_key, uint64_t* hi_key, int flags);
int qt_select_window(qt_handle_t* h, const double* sorted, long long n, const uint64_t* lo_key, const uint64_t* hi_key, int L,
                     int W, double* window, int flags);
int qt_select_finish(qt_handle_t* h, const double* windows, int N, int L, int W, long long n_total, const double* conf_levels,
                     double* out, int32_t* overflow, int flags);
/* R sorted runs stored back to back in runs (run_lengths[R]: always a HOST array) -> out: their merge in np.sort's
 * order (NaN last), by ceil(log2 R) merge-path passes.  out must not alias runs.  The values keep their bits; runs
 * sorted by np.sort (zeros interleaved, NaNs of either sign last) merge like runs from qt_sort_f64. */
int qt_merge_sorted(qt_handle_t* h, const double* runs, const int64_t* run_lengths, int R, double* out, int flags);

/* ---- f2: quantpy/stats.py:21-47 over a batch of trials (MomentInterval, interval.py:59-110) ----------------------
 * mean[b], var[b] of ||P (f_b - p)||^2 under multinomial noise, f_b[s][k] = counts[b][s][k] / ns[s] (interval.py:73,
 * :82), n_trials = the shots per setting (interval.py:89: n_measurements[0]), weights W = P^T P with
 * P = inv_matrix[rows][S*K] (the left inverse of the design matrix / dim, interval.py:75-87; W is formed on the matrix
 * cores).  For process tomography S = (input states) x (settings).  Up to S * K = 8192 rows one workgroup keeps the
 * frequencies of its trials in LDS; above that the counts are turned into frequencies first and take the kernels of
 * qt_moment_freq_batch (a three-qubit process with 'proj-set' has 64 x 216 = 13 824 rows).  S * K <= 32 768, where W
 * takes 8 GiB (QT_ERR_UNSUPPORTED beyond). */
int qt_moment_batch(qt_handle_t* h, const int64_t* counts, int B, int S, int K, const double* ns, const double* inv_matrix,
                    int rows, double n_trials, double* mean, double* var, int flags);
/* The same moments from frequencies given directly, freq[B][S*K]: the reference forms results / n_measurements[:, None]
 * in floating point (interval.py:70-90) and its sums (stats.py:21-47) take any real frequencies, e.g. expected counts
 * N p that are not integers.  W is split over the grid by columns (whole settings, or pieces of one when K > 256) and by
 * runs of settings; the workgroups' partial sums are added in a fixed order by a second kernel, without atomics: the
 * same input gives the same bits on every call, and a trial the same bits alone and in a batch.  LDS does not grow
 * with S, K or S * K; any S >= 1 and K >= 1 with S * K <= 32 768.  Fed counts / ns it returns the bits of
 * qt_moment_batch above 8192 rows; at or below, the two sum in different orders. */
int qt_moment_freq_batch(qt_handle_t* h, const double* freq, int B, int S, int K, const double* inv_matrix, int rows,
                         double n_trials, double* mean, double* var, int flags);

/* ---- f3: quantpy/tomography/interval.py:268-335 (PolytopeStateInterval: 2 * n_points cvxopt `solvers.lp` calls) -----
 * R x O dense linear programs that share one constraint matrix:
 *     minimise C[o] . x  subject to  A x <= b[r],  x in R^N free          (r < R, o < O)
 * A[M][N], C[O][N], b[R][M]; obj[R][O], x[R][O][N] (nullable: the final iterate), status[R][O] (qt_lp_status),
 * iters[R][O] (nullable: interior-point iterations of both phases).  One workgroup per program: primal-dual interior
 * point (Mehrotra predictor-corrector) on the normal matrix A^T diag(z / s) A, with a phase-1 program for a strictly
 * feasible start (csrc/qt_lp.h).  A streams from L2 in row blocks: M is not limited by LDS.  N <= 64 (n <= 3 qubits:
 * N = 4^n - 1), M >= N.  obj is +inf for INFEASIBLE, -inf for UNBOUNDED, NaN for NOT_CONVERGED.  When A is
 * numerically rank deficient (a pivot of the Cholesky factor of A^T A below 1e-12 of its diagonal entry) every program
 * reports NOT_CONVERGED.  Host-pointer calls return the number of programs whose status is not OPTIMAL. */
enum qt_lp_status {
  QT_LP_OPTIMAL = 0,       /* relative duality gap and scaled primal / dual residuals <= 1e-10 */
  QT_LP_INFEASIBLE = 1,    /* no x satisfies A x <= b (phase 1 converged to t* >= 0)           */
  QT_LP_UNBOUNDED = 2,     /* feasible iterates along which the objective diverges              */
  QT_LP_NOT_CONVERGED = 3  /* iteration cap (100 per phase), non-finite value or Cholesky breakdown */
};
int qt_lp_ineq_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                     double* obj, double* x, int32_t* status, int32_t* iters, int flags);

/* The same programs, arguments, statuses and return value for 1 <= N <= 255 (csrc/qt_lp_large.h): the polytope of a
 * two-qubit process (reference interval.py:338-418, N = 16^2 - 16 = 240) and of a four-qubit state (N = 255).  The
 * normal matrix (up to 256 x 256) lives in a per-workgroup slice of a global workspace (0.5 MB + 7 M doubles per
 * workgroup, at most 256 MB in all) and is factored by a blocked Cholesky in which a pivot not above 1e-11 of its
 * diagonal entry of H is replaced by that entry: without this the iteration breaks down on most polytope programs of
 * this size shortly before it converges.  N > 255 is QT_ERR_UNSUPPORTED, and so is an M whose seven M-vectors do not
 * fit the 256 MB beside one normal matrix (M > 4.7 million).  For N <= 64 both entry points accept the
 * program; their results agree to the solver's tolerance, not bit for bit (the sums run in another order). */
int qt_lp_ineq_large_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                           double* obj, double* x, int32_t* status, int32_t* iters, int flags);

/* The same programs, arguments, statuses and return value for 1 <= N <= 1023 (csrc/qt_lp_xl.h): the polytope of a
 * five-qubit state (N = 4^5 - 1; A is 7776 x 1023 with 'proj-set').  The normal matrix (up to 1024 x 1024, 8 MB) lives
 * in a per-workgroup slice of a global workspace and is formed on the FP64 matrix cores; the blocked Cholesky and its
 * pivot rule are those of qt_lp_ineq_large_batch.  A workgroup occupies a compute unit, so a call launches at most 256
 * of them and its workspace is 8 388 608 + 56 M bytes per workgroup, at most 4 GB in all (2.3 GB for 256 workgroups at
 * M = 7776; a call with fewer programs allocates for those only).  The workspace grows to the largest call and stays
 * with the handle until qt_destroy.  N > 1023 is QT_ERR_UNSUPPORTED, and so is an M whose seven M-vectors do not fit the
 * 4 GB beside one normal matrix (M > 76 million).  At 7776 x 1023 a program takes 3.7 s (187 ms per iteration, measured
 * on an MI355X: profiles/lp_xl_timing.txt) and 256 of them 5.0 s: callers split large batches into launches of about
 * 256 programs.  Below 256 variables the entry agrees with qt_lp_ineq_large_batch to the solver's tolerance, not bit
 * for bit. */
int qt_lp_ineq_xl_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                        double* obj, double* x, int32_t* status, int32_t* iters, int flags);

/* The primitives of one of the three LP kernels, run once on the caller's vectors: a test and diagnosis entry, not a
 * production path (a whole solve hides a wrong entry of H behind a few more iterations; this shows it).
 * kernel: 0 = qt_lp_ineq_batch's (N <= 64), 1 = qt_lp_ineq_large_batch's (N <= 255), 2 = qt_lp_ineq_xl_batch's
 * (N <= 1023); sizes are refused as by those entries (QT_ERR_ARG for N < 1 or M < N, QT_ERR_UNSUPPORTED above the
 * kernel's N or workspace).  Inputs: A[M][N]; w[M], the weights of the normal matrix; vm[M]; vn[n].  p1 (0 / 1) adds the
 * phase-1 column, -1 in every row: n = N + p1.  mode 0 factors as the kernel does inside a solve (plain Cholesky for
 * kernel 0; for 1 and 2 a pivot not above 1e-11 of its diagonal entry of H is replaced by that entry); mode 1 is the
 * kernels' rank test (no border: p1 must be 0; a pivot not above 1e-12 of its diagonal entry is a breakdown).
 * Outputs, each nullable:
 *   normal[n][n]  the lower triangle of H = A^T diag(w) A (bordered) as the kernel forms it, before factoring,
 *   factor[n][n]  the lower triangle of its Cholesky factor L (undefined where ok is 0),
 *   u[n]          A^T vm, and u[N] = sum(vm) with p1,
 *   ax[M]         A vn[0..N),
 *   solved[n]     (L L^T)^-1 vn (written only where ok is 1),
 *   ok[1]         1 if the factorisation succeeded, 0 on a breakdown.
 * The upper triangles of normal and factor are not written.  Before the launch the entry fills the kernel's workspace
 * slice and every non-null output with 0xFF bytes (a NaN in every double), and the kernel does the same to its LDS: a
 * primitive that reads an entry nothing wrote (the upper triangle of H, a column past n, a row past n of a partly
 * filled block) hands a NaN on, and what the call leaves unwritten stays all-ones.  One workgroup, on the handle's
 * workspace of the chosen kernel.  Returns 0. */
int qt_lp_pieces(qt_handle_t* h, int kernel, const double* A, int M, int N, const double* w, const double* vm,
                 const double* vn, int p1, int mode, double* normal, double* factor, double* u, double* ax, double* solved,
                 int32_t* ok, int flags);

/* ---- f4: quantpy/tomography/polytopes (the coverage study of arXiv:2109.04734, Fig. 1) over a batch of trials ------
 * A trial is a count table counts[b][R][K] with shots[r] per setting (for a process the output tomographs are stacked,
 * R = inputs x settings, and shots repeats the first tomograph's, as utils.py:11 broadcasts them);
 * f = clip(counts / shots[r], 1e-15, 1 - 1e-15) (verification.py:30, :66).  Counts are not validated against the shots.
 * Any R, K (csrc/qt_polytope.h picks the mapping from the shape alone, so splitting a batch over calls changes no bit);
 * every entry of shots must be positive and finite (QT_ERR_ARG).  B = 0 returns 0 and writes nothing.
 *
 * qt_polytope_confidence: conf[b][q] = count_confidence(deltas[b][q], f_b, shots) (utils.py:4-13).
 * qt_polytope_coverage: for every trial and level, delta = count_delta(levels[l], f_b, shots) (utils.py:16-27: 34
 * bisection steps) and hit = min(bound - truth) > -1e-15 with bound = clip(f + delta, 1e-15, 1 - 1e-15) when clip_b != 0
 * (test_qst, verification.py:33-34) and f + delta otherwise (test_qpt, verification.py:70-75); truth[R][K] = the true
 * outcome probabilities A x + W[:, 0] (verification.py:17-25, :52-60).  Outputs, each nullable (not all three):
 * deltas[B][L]; hits[B][L] (0 / 1); covered[L], to which the number of covering trials is ADDED (a study runs in chunks
 * of trials).  hits and covered need truth. */
int qt_polytope_confidence(qt_handle_t* h, const int64_t* counts, long long B, int R, int K, const double* shots,
                           const double* deltas, int Q, double* conf, int flags);
int qt_polytope_coverage(qt_handle_t* h, const int64_t* counts, long long B, int R, int K, const double* shots,
                         const double* levels, int L, const double* truth, int clip_b, double* deltas, uint8_t* hits,
                         long long* covered, int flags);

/* Metropolis-Hastings chains on the Cholesky parameters (mhmc.py:80-119 with `normalized_update`, used by
 * MHMCStateInterval, interval.py:735-750): C independent chains (the reference runs one), each on its
 * own counts[c][S][K]; x_init[C][D]; proposal increments deltas[C][T][D] and uniforms[C][T] drawn by the
 * caller (host RNG, reference order); chain[C][T][D] = state after every step, accepted[C][T].  n <= 5. */
int qt_mhmc_state(qt_handle_t* h, const int64_t* counts, int C, const double* x_init, const double* deltas,
                  const double* uniforms, int T, double step, double* chain, int32_t* accepted, int flags);

/* The random numbers of such a chain drawn on the device, defined by index (csrc/qt_sampler.h: mhmc_draw).  Global step
 * j of global chain c (j counts the burn-in steps first, then the sampling steps) owns the Philox4x32-10 stream
 * (key = seed, row = c, substream = 1 + j): counter {q, c low, c high, 1 + j}; substream 0 is qt_device_multinomial's.
 * Block q < D/2 (words w0..w3) holds the increments of parameters 2q and 2q + 1 by Box-Muller,
 *   u1 = u53(w0, w1), u2 = u53(w2, w3), r = sqrt(-2 log(1 - u1)), delta[2q] = r cos(2 pi u2), delta[2q + 1] = r sin(2 pi u2),
 * with u53(a, b) = ((a >> 5) 2^26 + (b >> 6)) / 2^53, and block q = D/2 the step's uniform u53(w0, w1).  Every number is
 * a pure function of (seed, c, j, index): no launch, batch position, rank count or lane enters it.  This keying is ABI,
 * like the row keying of qt_device_multinomial.  n <= 3 (n = 4, 5: QT_ERR_UNSUPPORTED); C = 0 or T = 0 returns 0.
 *
 * qt_mhmc_draws: deltas[C][T][D], uniforms[C][T] of chains first_chain .. first_chain+C-1, steps first_step ..
 * first_step+T-1 (first_step + T >= 2^32 - 1: QT_ERR_ARG) -- what qt_mhmc_state needs to run the same chain. */
int qt_mhmc_draws(qt_handle_t* h, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T,
                  double* deltas, double* uniforms, int flags);

/* C chains, chain i on counts[i][S][K] from x_init[i][D] (qt_chol_param of centres[i]), numbers as above for global
 * chain first_chain + i.  After the burn-in, post-burn step s is kept when s % thinning == 0 (mhmc.py:80-84): of the
 * kept states,  hits[i] = #{ thresholds[i] > hs_dst(unparam(x), centres[i]) }  (strict: a NaN never counts; unparam as
 * qt_chol_unparam, the distance as qt_hs_dist_dim), accepted[i] = accepted post-burn steps; dist[C][n_points] NULLABLE =
 * the kept distances in chain order.  centres[C][d][d][2], thresholds[C].  The steps are those of qt_mhmc_state (one
 * device function).  burn_steps >= 0, n_points >= 0, thinning >= 1 and burn_steps + n_points * thinning < 2^32 - 1, else
 * QT_ERR_ARG; n = 4, 5: QT_ERR_UNSUPPORTED; C = 0 returns 0 without a launch. */
int qt_mhmc_state_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* x_init,
                       const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                       int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags);
/* The same chains with the kept states measured in trace distance or infidelity (geometry.py:23-38, :41-56): every
 * argument as in qt_mhmc_state_hits, `metric` behind the handle as in qt_metric_dist_*.  The chain, its Philox keying and
 * the kept-step rule are the device functions of qt_mhmc_state_hits: for the same (seed, first_chain, counts, x_init)
 * accepted[] is bit-identical to that entry's.  The distance of a kept state is the value qt_metric_dist_group_batch
 * returns for unparam(x) (L L^dagger as qt_chol_unparam forms it) and centres[i], by the same device functions:
 *   both arguments taken as HERMITIAN, the imaginary parts of the diagonals dropped,
 *   QT_METRIC_TRACE       sum_k |lambda_k(R - C)| / 2,
 *   QT_METRIC_INFIDELITY  1 - (sum_k sqrt(max(mu_k, 0)))^2, mu the eigenvalues of the Hermitian part of S R S, S the
 *                         clipped Hermitian root of the centre (the roots of the C centres are made once per call, by the
 *                         set-up kernel of qt_metric_dist_group_batch into its workspace: the same root bits),
 *   a value below 1e-15 returned as 0; a NaN or infinity in centres[i] gives NaN distances, which never count as hits
 *   (hits[i] = 0), and touches no other chain.
 * A chain's bits depend on its own inputs and its global chain index alone: not on C or its place in the batch.
 * hits[i] = #{ kept : thresholds[i] > distance } (strict); accepted, dist NULLABLE as above.
 * QT_ERR_ARG: everything qt_mhmc_state_hits refuses, and a metric other than QT_METRIC_TRACE / QT_METRIC_INFIDELITY (the
 * Hilbert-Schmidt distance stays with qt_mhmc_state_hits); n = 4, 5: QT_ERR_UNSUPPORTED before any launch; C = 0 returns 0
 * without a launch. */
int qt_mhmc_state_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                              const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                              int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                              double* dist, int flags);

/* qt_mhmc_draws with the vector length given instead of read from the handle, on a handle of any size (no POVM is read):
 * deltas[C][T][dim], uniforms[C][T] by the definition stated at qt_mhmc_draws with D = dim -- the same kernel, so
 * dim = 4^n on an n <= 3 handle gives the bits of qt_mhmc_draws.  dim even, 2 <= dim <= 4096, else QT_ERR_ARG;
 * first_step + T >= 2^32 - 1: QT_ERR_ARG; C = 0 or T = 0 returns 0.  With dim = 256, 1024 it is what qt_mhmc_state needs
 * to run the chain of qt_mhmc_state_large_hits at n = 4, 5. */
int qt_mhmc_draws_dim(qt_handle_t* h, int dim, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T,
                      double* deltas, double* uniforms, int flags);

/* qt_mhmc_state_hits for n = 4, 5 handles: every argument, the kept-step rule, hits (strict, a NaN threshold or distance
 * never counts), accepted and the NULLABLE dist as there; numbers as qt_mhmc_draws_dim(dim = 4^n) gives them for global
 * chain first_chain + i.  One workgroup of 4^n threads per chain runs the steps of qt_mhmc_state at these sizes operand
 * for operand -- that entry on the numbers of qt_mhmc_draws_dim accepts exactly the same steps -- forms a kept state as
 * qt_chol_unparam does and its distance to centres[i] as qt_hs_dist_dim defines it (the order of the d^2-term sum is the
 * workgroup's: within 10 d^2 2^-52 of that entry).  No LDS beyond the chain's own.
 * QT_ERR_ARG as qt_mhmc_state_hits; n <= 3: QT_ERR_UNSUPPORTED before any launch (the entry there is
 * qt_mhmc_state_hits); C = 0 returns 0 without a launch. */
int qt_mhmc_state_large_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* x_init,
                             const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                             int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags);
/* qt_mhmc_state_metric_hits for n = 4, 5 handles: the chains of qt_mhmc_state_large_hits (accepted[] bit-identical to that
 * entry's) with a kept state measured as qt_metric_dist_dim(dim = 2^n) measures unparam(x) against centres[i], by the same
 * device functions in the kernel that holds the state; the infidelity's roots of the C centres are made once per call by
 * the set-up kernel of qt_metric_dist_dim into its workspace (the same root bits).  A NaN or infinity in centres[i] gives
 * NaN distances and hits[i] = 0, and touches no other chain.  QT_ERR_ARG: everything qt_mhmc_state_large_hits refuses and
 * an unknown metric; n <= 3: QT_ERR_UNSUPPORTED (the entry there is qt_mhmc_state_metric_hits). */
int qt_mhmc_state_large_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                    const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                    int burn_steps, int n_points, int thinning, double step, int64_t* hits,
                                    int64_t* accepted, double* dist, int flags);

/* ---- a11-a15: quantpy/tomography/process.py -------------------------------------------------- */
/* Process tomography of an n-qubit channel (handle created with n_qubits = n; n <= 3: 'lifp', the projections and
 * what builds on them ('states', the bootstrap), 'pgdb' and the process chain all run for n <= 3; at n = 3 through the
 * Kronecker factors of the design matrix).
 * qt_process_setup: input states in_states[D][d][d][2] (process.py:79), the weighted POVM of
 * qt_set_povm (call it first) -> design matrix rows vec(rho_in (x) E_m^T) (process.py:203-208),
 * its left inverse (process.py:210), and the partial-trace operator (routines.py:47-50). */
int qt_process_setup(qt_handle_t* h, const double* in_states, int flags);
/* lifp_oper[D*M][D^2][2] (nullable) and its left inverse [D^2][D*M][2] (nullable) */
int qt_process_get_operators(qt_handle_t* h, double* lifp_oper, double* lifp_oper_inv, int flags);
/* n = 3 (and n = 2 beside the dense form): the design matrix Kronecker-factored, L = (V_S (x) V_P) Pi^T with V_S = [vec rho_s] (D x D) and
 * V_P = [vec E_m] (M x D, column e d + b <-> E_m[e][b]), so that L^+ = Pi (V_S^+ (x) V_P^+) (plain transposes,
 * routines.py:69-71): vs_pinv[D][D][2], vp_pinv[D][M][2] (each nullable).  Entry [(c d + e) D + (a d + b)][s M + m] of
 * the reference's `_lifp_oper_inv` is vs_pinv[a d + c][s] * vp_pinv[e d + b][m]. */
int qt_process_get_factors(qt_handle_t* h, double* vs_pinv, double* vp_pinv, int flags);
/* n = 2 keeps BOTH forms: the dense operator (qt_process_get_operators, 'pgdb', the process chain) and, when M % 4 == 0,
 * the factors, which qt_lifp_batch multiplies by (34 matrix instructions per process instead of 288; same Choi matrix
 * to rounding).  on != 0 makes qt_lifp_batch use the dense left inverse instead (A/B measurements, tests). */
int qt_process_prefer_dense(qt_handle_t* h, int on);
/* counts[B][D][S][K] -> choi[B][D][D][2] (process.py:284-289); cptp != 0 applies the Dykstra
 * projection of process.py:231-257 (n_iter <= 1000, stop 1e-12); iters[B] (nullable) */
int qt_lifp_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, double* choi, int32_t* iters,
                  int32_t* status, int flags);
/* The resample loop of the process bootstrap (interval.py:673-682) in one pass: qt_lifp_batch, and
 * dist[B] = hs_dst(Choi_b, centre) as qt_hs_dist_dim computes it (sqrt(|sum_ij D_ij D_ji|) / sqrt(2), no conjugation, 0
 * below 1e-15), for centre[D][D][2] (need not be Hermitian).  choi is NULLABLE: without it no matrix leaves the device.
 * With it, choi / iters / status are bit-identical to qt_lifp_batch's.  n <= 2 on the default paths forms the distance
 * in the kernel that holds the matrix (the order of its D^2-term sum is then that kernel's); every other path stores
 * the matrices (in a handle workspace when choi is null, a slice at a time: QT_OPT_LIFP_DIST_SLICE) and runs
 * qt_hs_dist_dim's kernel on them: the same bits as the two calls. */
int qt_lifp_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, const double* centre, double* choi,
                       double* dist, int32_t* iters, int32_t* status, int flags);
/* The bootstrap coverage study for processes (quantpy/metrics.py:282-316: every trial t bootstraps around ITS OWN Choi
 * estimate): qt_lifp_dist_batch with a table centres[G][D][D][2], dist[b] = hs_dst(Choi_b, centres[b % G]).  The batch is
 * resample-major, counts[r * G + t] = resample r of trial t -- the order qt_device_multinomial writes with
 * period = G * D * S and qt_process_born_probs' table as pvals.  G >= 1 (else QT_ERR_ARG); G = 1 is qt_lifp_dist_batch.
 * Everything else -- choi NULLABLE, iters, status, the choice of path from the whole batch, the slices -- as there. */
int qt_lifp_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, const double* centres, int G, double* choi,
                             double* dist, int32_t* iters, int32_t* status, int flags);
/* The outcome probabilities of G channels given by their Choi matrices choi[G][D][D][2], on the D input states of
 * qt_process_setup (requires qt_set_povm* and qt_process_setup):
 *   p[G][D][S][K] = clip(Born(povm, E_g(rho_i)), 0, 1),   E_g(rho) = Tr_in[(rho^T (x) I) C_g]  (channel.py: Channel.transform)
 * Row (g * D + i) * S + s is one multinomial's pvals: the table qt_device_multinomial reads with period = G * D * S. */
int qt_process_born_probs(qt_handle_t* h, const double* choi, int G, double* p, int flags);
/* 'pgdb' (process.py:291-308): projected gradient descent with backtracking from the fully mixed Choi
 * matrix, raw counts as weights, every arithmetic quirk of the reference kept (see qt_process.h).
 * stop_rule 0 = the reference's loop exit (leaves at the first step that lowers the NLL by more than
 * tol and returns the point BEFORE it -- in practice the starting point); 1 = accept steps until the
 * decrease falls below tol.  iters[B], status[B] nullable. */
int qt_pgdb_batch(qt_handle_t* h, const int64_t* counts, int B, int n_iter, double tol, int stop_rule, double* choi,
                  int32_t* iters, int32_t* status, int flags);
/* The pieces of ONE 'pgdb' iteration at the points choi_in[B][D][D][2] (process.py:296-298), for checking the
 * factored n = 3 operators against the reference's dense ones: probas[B][D*M] = Re(L c), grad[B][D][D][2] =
 * -L^H (n / p) laid out like the Choi matrix (entry [i][j] = component j D + i of the reference's column-stacked
 * vector), projected[B][D][D][2] = P_CPTP(c - grad / mu).  Each output nullable.  n = 3 only (n <= 2 keeps the whole
 * loop in one kernel, tested through its results). */
int qt_pgdb_pieces(qt_handle_t* h, const int64_t* counts, int B, const double* choi_in, double* probas, double* grad,
                   double* projected, int flags);
/* Metropolis-Hastings chains on the Choi vector (MHMCProcessInterval, interval.py:808-836): proposals
 * P_CPTP(x + step * delta), target exp(-nll) with the raw counts.  counts[C][D][S][K], choi_init[C][D][D][2],
 * deltas[C][T][D*D] (real, indexed like the column-stacked Choi vector), uniforms[C][T];
 * chain[C][T][D][D][2] = Choi matrix after every step, accepted[C][T]. */
int qt_mhmc_process(qt_handle_t* h, const int64_t* counts, int C, const double* choi_init, const double* deltas,
                    const double* uniforms, int T, double step, double* chain, int32_t* accepted, int flags);

/* The random numbers of such a chain drawn on the device: the definition stated at qt_mhmc_draws with the vector length
 * D replaced by D^2 (D = 4^n, the Choi vector has D^2 real increments).  Global step j of global chain c owns the
 * Philox4x32-10 stream (key = seed, row = c, substream = 1 + j), counter {q, c low, c high, 1 + j}: block q < D^2/2 holds
 * the increments of the column-stacked entries 2q and 2q + 1 (Box-Muller, as there), block q = D^2/2 the step's uniform
 * u53(w0, w1).  This keying is ABI.  A state chain (qt_mhmc_draws) and a process chain with the same (seed, chain) read
 * overlapping Philox blocks -- blocks q < D/2 of a step are the same words in both, and the state chain's uniform is the
 * u1 of the process chain's block D/2 -- so their numbers are NOT independent: never run both under one key (the studies
 * of metrics do not: each derives its key from its own seed and runs one kind of chain).
 * Both entries need qt_set_povm* and qt_process_setup, and n <= 2 (n = 3, whose chain is four launches per step:
 * QT_ERR_UNSUPPORTED before any launch).
 *
 * qt_mhmc_process_draws: the numbers of qt_mhmc_process_hits written out, deltas[C][T][D*D], uniforms[C][T] of chains
 * first_chain .. first_chain+C-1, steps first_step .. first_step+T-1 (first_step + T >= 2^32 - 1: QT_ERR_ARG; C = 0 or
 * T = 0 returns 0) -- what qt_mhmc_process needs to run the same chain. */
int qt_mhmc_process_draws(qt_handle_t* h, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T,
                          double* deltas, double* uniforms, int flags);
/* C chains, chain i on counts[i][D][S][K] from choi_init[i][D][D][2], numbers as above for global chain first_chain + i,
 * the steps those of qt_mhmc_process (one device function).  After the burn-in, post-burn step s is kept when
 * s % thinning == 0 (mhmc.py:80-84).  Of the kept states X,
 *   hits[i] = #{ thresholds[i] > hs_dst(Re(X), centres[i]) }   (strict: a NaN never counts),
 * the distance of the REAL PART (mhmc.py:66 stores the samples in a real array) formed as qt_hs_dist_dim forms it:
 * Delta = Re(X) - centre, sqrt(|sum_ij Delta_ij Delta_ji|) / sqrt(2), 0 below 1e-15.  accepted[i] = accepted post-burn
 * steps; dist[C][n_points] NULLABLE = the kept distances in chain order.  centres[C][D][D][2], thresholds[C].
 * burn_steps >= 0, n_points >= 0, thinning >= 1 and burn_steps + n_points * thinning < 2^32 - 1, else QT_ERR_ARG;
 * C = 0 returns 0 without a launch. */
int qt_mhmc_process_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* choi_init,
                         const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                         int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags);
/* The same chains with the REAL PART of the kept points measured in trace distance or infidelity (geometry.py:23-38,
 * :41-56): every argument as in qt_mhmc_process_hits, `metric` behind the handle as in qt_metric_dist_*.  The chain, its
 * Philox keying and the kept-step rule are the device functions of qt_mhmc_process_hits: for the same (seed, first_chain,
 * counts, choi_init) accepted[] is bit-identical to that entry's.  The distance of a kept point X is the value
 * qt_metric_dist_dim returns at dim = D = 4^n for Re(X) and centres[i], by the same device functions:
 *   both arguments taken as HERMITIAN, the imaginary parts of the diagonals dropped,
 *   QT_METRIC_TRACE       sum_k |lambda_k(Re(X) - C)| / 2,
 *   QT_METRIC_INFIDELITY  1 - (sum_k sqrt(max(mu_k, 0)))^2, mu the eigenvalues of the Hermitian part of S Re(X) S, S the
 *                         clipped Hermitian root of the centre (made once per call by the set-up kernel of
 *                         qt_metric_dist_dim into its workspace: the same root bits),
 *   a value below 1e-15 returned as 0; a NaN or infinity in centres[i] gives NaN distances, which never count as hits
 *   (hits[i] = 0), and touches no other chain.
 * (A Choi matrix here has trace 2^n, so the infidelity of two of them is 1 - (~2^n)^2 < 1e-15 and comes back as 0, as
 * geometry.py:52-54 returns it: meaningful only for centres scaled to unit trace.)
 * A chain's bits depend on its own inputs and its global chain index alone: not on C or its place in the batch.
 * hits[i] = #{ kept : thresholds[i] > distance } (strict); accepted, dist NULLABLE as above.
 * QT_ERR_ARG: everything qt_mhmc_process_hits refuses, and a metric other than QT_METRIC_TRACE / QT_METRIC_INFIDELITY;
 * n = 3: QT_ERR_UNSUPPORTED before any launch; C = 0 returns 0 without a launch; a missing POVM or qt_process_setup
 * fails as there. */
int qt_mhmc_process_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                const double* choi_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                                double* dist, int flags);
/* qt_mhmc_process_hits for n = 3 handles: every argument, the kept-step rule (post-burn step s is kept when
 * s % thinning == 0), hits (strict: a NaN threshold or distance never counts), accepted, the NULLABLE dist[C][n_points],
 * the argument errors (QT_ERR_ARG: burn_steps < 0, n_points < 0, thinning < 1, burn_steps + n_points * thinning >=
 * 2^32 - 1, a null array with C > 0) and C = 0 (returns 0 without a launch) as there.  counts[C][D][S][K],
 * centres[C][D][D][2], choi_init[C][D][D][2], thresholds[C], D = 64.
 * Numbers: chain i runs on counts[i] from choi_init[i] with the numbers of global chain first_chain + i at vector length
 * 4096, as qt_mhmc_draws_dim(dim = 4096) writes them out (no draws entry of its own is needed: that one reads no POVM and
 * serves any handle): increment l of global step j belongs to the column-stacked entry l of the Choi vector -- element
 * (row, col) of the row-major matrix takes l = 64 col + row, how qt_mhmc_process indexes `deltas` -- and Philox block
 * q = 2048 holds the step's uniform.
 * Steps: those of qt_mhmc_process at n = 3, a launch family per step -- the proposal x + step * delta (one fused
 * multiply-add per element) with its draws, the CPTP projection (1000 iterations, tol 1e-12), the model and the NLL, the
 * accept rule u <= exp(nll(x) - nll(x')) with its draw -- through the same device functions: for the same (seed,
 * first_chain, counts, choi_init) accepted[i] equals, exactly, what qt_mhmc_process accepts behind the burn-in on the
 * numbers of qt_mhmc_draws_dim.  The chain's point stays on the device; per chain only hits, accepted and dist leave it.
 * Distance: hs_dst(Re(X), centres[i]) of a kept state X is formed by the kernel that decides the step, as qt_hs_dist_dim
 * forms it (Delta = Re(X) - centre, sqrt(|sum_ij Delta_ij Delta_ji|) / sqrt(2), 0 below 1e-15) with its own order of the
 * 4096-term sum: within 1e-12 absolute of qt_hs_dist_dim on the written-out chain for distances below 1 (for a
 * Hermitian centre the terms are non-negative, so any order is within 4096 * 2^-52 relative on the sum, half of that on
 * the root).
 * A chain's bits depend on its own inputs and its global chain index alone: not on C or its place in the batch.
 * Workspace is O(min(C, slice)), about 0.6 MB per chain of a slice (the current point, the trial and its projection at
 * 64 KB each, 320 KB of the projection's own, the NLL's tile partials; the metric entry adds 64 KB for the kept state and,
 * for the infidelity, 64 KB per chain of the CALL for the centres' roots): the chains run in slices of
 * QT_OPT_MHMC_PROCESS_SLICE chains (default 1024), one after the other on the handle's stream, with plain launches and
 * no host synchronisation.  The same bits whatever the slice.
 * n <= 2 (and n >= 4): QT_ERR_UNSUPPORTED before any launch, the text naming qt_mhmc_process_hits, the entry for n <= 2;
 * then a missing POVM, then a missing qt_process_setup: QT_ERR_STATE, as there. */
int qt_mhmc_process_large_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* choi_init,
                               const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                               int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags);
/* qt_mhmc_process_metric_hits for n = 3 handles: the chains of qt_mhmc_process_large_hits (accepted[] bit-identical to
 * that entry's) with the REAL PART of every kept point measured in trace distance or infidelity; `metric` behind the
 * handle as in qt_metric_dist_*, every other argument as there.  On a kept step the deciding kernel leaves Re(X), with
 * zero imaginary parts, in a per-chain buffer, qt_metric_dist_mat's kernel for dim = 64 measures it against centres[i]
 * (the infidelity's roots of the C centres made once per call by that entry's set-up kernel), and a tally kernel
 * compares with thresholds[i] (strict), counts the hit and writes dist[i][k]: the distances are bit-identical to
 * qt_metric_dist_mat(dim = 64) on the real parts of the written-out chain.  Conventions of the two metrics, the
 * degenerate infidelity of trace-2^n Choi matrices (every distance 0) and the NaN rule (a NaN or infinity in centres[i]
 * gives NaN distances and hits[i] = 0, and touches no other chain) as in qt_mhmc_process_metric_hits.
 * QT_ERR_ARG: everything qt_mhmc_process_large_hits refuses, and a metric other than QT_METRIC_TRACE /
 * QT_METRIC_INFIDELITY; n <= 2: QT_ERR_UNSUPPORTED before any launch (the entry there is qt_mhmc_process_metric_hits);
 * a missing POVM or qt_process_setup, C = 0, determinism, workspace and slices as in qt_mhmc_process_large_hits. */
int qt_mhmc_process_large_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                      const double* choi_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                      int burn_steps, int n_points, int thinning, double step, int64_t* hits,
                                      int64_t* accepted, double* dist, int flags);
/* projections alone (process.py:231-278): mode 0 = CPTP (Dykstra), 1 = TP, 2 = CP */
int qt_cptp_project_batch(qt_handle_t* h, const double* choi_in, int B, int mode, int n_iter, double tol,
                          double* choi_out, int32_t* iters, int flags);
/* The 'states' process estimator (process.py:316-327) on B trials of reconstructed output states,
 * states[B][D][d][d][2] in the order of qt_process_setup's input states, n <= 3:
 *     C_b[(i,k)][(j,l)] = sum_s weights[(i,j)][s] rho_b,s[k][l]        (row index i d + k, column index j d + l)
 * with weights[D][D][2], row (i,j) = i d + j and column s, built by the caller:
 * weights[(i,j)][s] = sum_e unit_e[i][j] c_e,s for the coordinates c_e of the single-entry matrices in the input basis
 * and unit_e = sum_s c_e,s rho_in,s -- the reference's sum_e unit_e (x) sum_s c_e,s rho_s.  weights is in the pointer
 * space of the other arguments.  Every entry of C_b is one chain of fused multiply-adds over s = 0 .. D - 1.
 * cptp = 0: assembly only; projected[B] and iters[B] (both NULLABLE) are zero.
 * cptp != 0: the conditional projection of the reference.  A trial that passes the test of qt_choi_is_cptp_batch
 * (atol = 1e-5) keeps its assembled matrix bit for bit, projected[b] = 0, iters[b] = 0.  A trial that fails receives
 * exactly what qt_cptp_project_batch(mode 0, n_iter 1000, tol 1e-12) returns for its assembled matrix, bit for bit,
 * with its iteration count, projected[b] = 1.  The failing trials are compacted on the device and projected in one
 * launch; their NUMBER is read back to size it, so with cptp the call waits for the handle's stream once per 128 MB of
 * Choi matrices (524 288 trials at n = 1, 32 768 at n = 2, 2048 at n = 3), also with QT_DEVICE_PTR.
 * A trial's bits depend on its own inputs only, not on B or its place in the batch.
 * n = 4, 5: QT_ERR_UNSUPPORTED before any launch; a missing POVM or qt_process_setup fails as qt_lifp_batch does;
 * B = 0 returns 0 without a launch. */
int qt_states_choi_batch(qt_handle_t* h, const double* states, int B, const double* weights, int cptp, double* choi,
                         int32_t* projected, int32_t* iters, int flags);
/* The same call plus dist[b] = hs_dst(C_b, centres[b % G]) for a table centres[G][D][D][2], formed by qt_hs_dist_dim's
 * kernel on the final matrices: the bootstrap coverage study of the 'states' estimator, with the conventions of
 * qt_lifp_dist_group_batch (resample-major batch, G >= 1 else QT_ERR_ARG).  choi is NULLABLE: without it no matrix leaves
 * the device, and the matrices of one 128 MB slice at a time live in a handle workspace. */
int qt_states_choi_dist_group_batch(qt_handle_t* h, const double* states, int B, const double* weights, int cptp,
                                    const double* centres, int G, double* choi, double* dist, int32_t* projected,
                                    int32_t* iters, int flags);
/* The device form of Channel.is_cptp(atol) (channel.py:144-157) on arbitrary matrices choi[B][D][D][2], n <= 3 (no POVM
 * needed): ok[b] = 1 when
 *   - every entry of choi[b] is finite,
 *   - R[i][j] = sum_k C[(i,k)][(j,k)] has |R - 1| <= atol + 1e-5 |1| element by element on the complex modulus
 *     (np.allclose's rule: rtol at its default 1e-5, so the diagonal gets 1e-5 more than the off-diagonal), and
 *   - the smallest eigenvalue of the Hermitian part (C + C^H) / 2 is >= -atol, decided by an L D L^H factorisation of
 *     Herm(C) + atol 1 with a positive-pivot test;
 * else ok[b] = 0.  CONTRACT: the flag equals the host's is_cptp whenever the smallest eigenvalue and the largest
 * trace-preservation residual are both farther than 1e-9 from their thresholds; inside that band either answer is
 * allowed.  atol >= 0 and finite, else QT_ERR_ARG; n = 4, 5: QT_ERR_UNSUPPORTED; B = 0 returns 0 without a launch. */
int qt_choi_is_cptp_batch(qt_handle_t* h, const double* choi, int B, double atol, int32_t* ok, int flags);

#ifdef __cplusplus
}
#endif
#endif /* QTOMO_H */
