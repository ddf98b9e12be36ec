// libqtomo.so -- C ABI (include/qtomo.h) over the HIP kernels in qt_small.h / qt_ops.h /
// qt_process.h.  gfx950 only.  There is no CPU implementation behind these entry points.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/qtomo.h"
#include "qt_large.h"
#include "qt_lp.h"
#include "qt_lp_large.h"
#include "qt_lp_xl.h"
#include "qt_metric_dim.h"
#include "qt_metric_dim64.h"
#include "qt_mhmc_state.h"
#include "qt_mhmc_state_large.h"
#include "qt_mle_small.h"
#include "qt_ops.h"
#include "qt_polytope.h"
#include "qt_process.h"
#include "qt_process64.h"
#include "qt_process_wave16.h"
#include "qt_product_tables.h"
#include "qt_sampler.h"
#include "qt_small.h"
#include "qt_states_choi.h"
#include "qt_mhmc_process64.h"  // (behind the older headers: its kernels are laid out behind theirs)

// the kernels' names (qt_linesearch.h) for the trial statuses of the public header
#define QT_SAME_STATUS(name) static_assert((int)qt::TRIAL_##name == (int)QT_TRIAL_##name, "qt::TrialStatus is QT_TRIAL_*")
QT_SAME_STATUS(OK);
QT_SAME_STATUS(NOT_PD);
QT_SAME_STATUS(LINESEARCH);
QT_SAME_STATUS(MAXITER);
QT_SAME_STATUS(NAN);
QT_SAME_STATUS(SHOTS);
#undef QT_SAME_STATUS

namespace {

#ifdef QT_PHASE_TIMING
int g_host_diag = 0;  // profile build: compile-time variant of k_lifp_gemm to launch (qt_debug_set_diag)
#endif
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(QT_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

constexpr int kStageBufs = 10;  // arrays one host-pointer call may stage (qt_lp_pieces: four inputs and six outputs)

// What qt_process_setup keeps of the design matrix L (rows vec(rho_s (x) E_m^T)).  n <= 2 keeps it dense (`lifp` ..
// `pinvR`); n = 3 keeps only the left inverses of its Kronecker factors (qt_process64.h: `factored`); n = 2 builds those
// next to the dense form when the POVM allows (`factors` without `factored`).
struct ProcessState {
  DevBuf in_states;  // [D][d][d] complex
  DevBuf emats;      // [M][d][d] complex POVM elements
  DevBuf lifp;       // [D*M][D^2] complex design matrix
  DevBuf pinv;       // [D^2][D*M] complex: its left inverse
  DevBuf pinvT;      // [D*M][D^2] complex: the transpose of that
  DevBuf pinvR;      // the same with each row's D^2 entries in ROW-major Choi order (k_lifp_gemm's operand: its product
                     // columns are then the doubles of choi[b] in order); built for n = 2 only
  DevBuf vs_pinv;    // [D][D] complex: left inverse of V_S = [vec rho_s]
  DevBuf vp_pinv;    // [D][M] complex: left inverse of V_P = [vec E_m] (index e d + b)
  DevBuf vp_pinvT;   // [M][D] complex: its transpose, the right-hand operand of T = F V_P^+^T
  DevBuf vp_perm;    // [groups][M][32] real: the same, 16 columns (re | im) per group in the order k_lifp64 (n = 3:
                     // 4 groups) / k_lifp16 (n = 2: 1 group) store them
  bool factored = false;  // the dense form was not built: the factors are all there is
  bool factors = false;   // vs_pinv, vp_pinv, vp_pinvT hold regular left inverses
  bool perm = false;      // ... and vp_perm their permuted copy: qt_lifp_batch takes the matrix-core kernels
  void release() {
    factored = factors = perm = false;
    for (DevBuf* b : {&in_states, &emats, &lifp, &pinv, &pinvT, &pinvR, &vs_pinv, &vp_pinv, &vp_pinvT, &vp_perm}) b->release();
  }
};

// What a registration (qt_set_povm / qt_set_povm_product) says about the POVM.  PovmState::reset assigns a fresh one, so
// a member added here is forgotten with the rest.  A registration fills it in as it goes and sets `registered` -- and,
// for a product POVM, `prod` -- as its last step: one that returns an error leaves a handle without a POVM.
struct PovmDesc {
  bool registered = false;
  double ns_tot = 0.0;  // sum of the registered shots per setting
  double ns_max = 0.0;  // the largest of them (product POVMs): the n >= 4 count cache holds 32-bit counts
  // The dense operands A, A^T, A', A'^T ([M][D] each: 64 MB at n = 5) exist when `dense_ready`; a product POVM at n >= 4
  // never reads them and builds them only on demand (ensure_dense: A from the one-qubit table unless `a_loaded`),
  // likewise the dense left inverse (`pinv_ready`, compute_dense_pinv).
  bool a_loaded = false, dense_ready = false, pinv_ready = false;
  int S1 = 0, K1 = 0;       // a product POVM's one-qubit factor: S1 settings of K1 outcomes, table T [S1 K1][4]
  qt::ProductView prod{};   // the product description as the kernels take it: pointers into the buffers below
  int paired_tables = 0;    // what qt_set_povm_product found: bit 0 = T is paired, bit 1 = pinv(T)^T is
  bool image_ready = false;  // `image` holds the table image (qt::SpecArgs::image: built when both tables are paired)
};

// The registered POVM: its description and the device memory that description points into, which outlives it for the
// next registration to reuse (DevBuf::ensure).
struct PovmState : PovmDesc {
  DevBuf Ns;                                // [S] shots per setting
  DevBuf A, AT, Aw, AwT, Pinv, PinvT;       // dense operands and left inverse
  DevBuf T, P1, P1T;                        // [R1][4] one-qubit table, [4][R1] its left inverse, [R1][4] the transpose
  DevBuf wrow, rmap, rinv, fwd, bwd, last;  // qt_product_tables.h
  DevBuf image;
  void reset() { static_cast<PovmDesc&>(*this) = PovmDesc{}; }
  void release() {
    reset();
    for (DevBuf* b : {&Ns, &A, &AT, &Aw, &AwT, &Pinv, &PinvT, &T, &P1, &P1T, &wrow, &rmap, &rinv, &fwd, &bwd, &last, &image})
      b->release();
  }
};

}  // namespace

struct qt_handle {
  int device = 0, nq = 0, d = 0, D = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_sync = nullptr;
  // Pinned host mailbox for the small transfers of host-pointer calls (counts of a few trials in, rho / nit / status
  // out): hipMemcpyAsync from / to pageable memory blocks the caller ~10 us per copy, a one-trial qt_mle_batch makes six.
  // Through pinned memory they are asynchronous; outputs are copied to the caller's arrays once the stream has been
  // waited for (Call::done).  Transfers above kMailMax, or when the box is full, take the direct route.
  char* mail = nullptr;
  size_t mail_used = 0;
  // The registered POVM (PovmState).  Its shape stays here, written by begin_povm alone: the whole file reads h->M.
  PovmState povm;
  int S = 0, K = 0, M = 0;
  DevBuf info;
  // packed row digits of the Kronecker assembly (k_povm_kron), cached per (S1, K1): qt_povm_kron's cache, which says
  // nothing about the registered POVM
  DevBuf kron_dig;
  int kron_S1 = 0, kron_K1 = 0;
  // staging for host-pointer calls: one buffer per array of a call, in the order the call registers them (Call)
  DevBuf stage[kStageBufs];
  DevBuf aug;      // [cols][2 cols] Gauss-Jordan workspace of enqueue_left_inverse
  DevBuf proc_ws;  // k_cptp_project64: Dykstra's p, q, y, x and the clip's input (project)
  DevBuf born_ws;       // qt_process_born_probs: the output states E_g(rho_i) and, behind them, their Bloch vectors
  DevBuf lifp_dist_ws;  // qt_lifp_dist_batch without `choi`: one slice's Choi matrices, where k_hs_dist reads them
  DevBuf gram;  // qt_moment_batch: P^T P
  DevBuf moment_freq, moment_part, moment_qpart;  // k_moment_cols: counts / ns, the blocks' partial sums, Q_ab in pieces
  DevBuf lp_ws;  // qt_lp_ineq_batch: six M-vectors per workgroup
  DevBuf lp_large_ws;  // qt_lp_ineq_large_batch: the normal matrix and seven M-vectors per workgroup
  // qt_lp_ineq_xl_batch: the same with an 8 MB normal matrix, one workgroup per compute unit; up to 2.3 GB after a call
  // with 256 five-qubit programs, kept until qt_destroy like every workspace here
  DevBuf lp_xl_ws;
  DevBuf poly_ws;  // qt_polytope_coverage: hits[B][L] when the caller wants only the counts
  DevBuf metric_ws;  // qt_metric_dist_group_batch / _dim / _mat, infidelity: the Hermitian roots of the call's G centres
  DevBuf mhmc_parked;  // qt_mhmc_process_large_metric_hits: a slice's kept states Re(X) and, behind them, their distances
  // MLE hand-off between k_mle_start and k_mle_bfgs
  DevBuf ws_x, ws_g, ws_f, ws_act;
  // BFGS (s, y) history of the n >= 4 kernels (max_iter x 2 D doubles per trial of a chunk)
  DevBuf hess;
  // radix-sort double buffer + temporary storage (qt_sort_f64)
  DevBuf sort_alt, sort_tmp;
  // process tomography
  ProcessState proc;
  bool proc_set = false;  // `proc` describes the current POVM: a set-up succeeded after the last qt_set_povm
  bool proc_dense = false;  // qt_process_prefer_dense: qt_lifp_batch multiplies by the dense left inverse where it has a choice

  bool check_shots = true;  // qt_set_option(QT_OPT_SHOTS_CHECK) / QTOMO_SKIP_SHOTS_CHECK=1 at qt_create
  int fused_max_waves = 1024;  // qt_set_option(QT_OPT_MLE_FUSED_MAX_WAVES): largest batch (in trial-waves) of k_mle_fused
  int lifp_dist_slice = 0;  // qt_set_option(QT_OPT_LIFP_DIST_SLICE): processes per slice of qt_lifp_dist_batch (0: the byte bound's)
  int mhmc_process_slice = 0;  // qt_set_option(QT_OPT_MHMC_PROCESS_SLICE): chains per slice of qt_mhmc_process_large_hits (0: 1024)
  bool paired_stages = true;  // qt_set_option(QT_OPT_PAIRED_STAGES): let paired tables take their own stages (n <= 3)
  // qt_set_option(QT_OPT_MLE_SPECIALISE): let an eligible POVM take the specialised MLE kernels (GENERIC = false, n <= 3)
  bool mle_specialise = true;
  bool last_mle_spec = false;  // which instantiation the last MLE launch took (qt_get_mle_specialised)
  // qt_set_option(QT_OPT_MLE_HELPER_WAVE): let the one-launch 'lin' start at n = 3 run k_mle_fused_hw (a helper wavefront
  // per trial, which runs the single-negative lift on speculation and a lifted trial's second Cholesky sweep)
  bool mle_helper_wave = true;
  bool last_mle_helper = false;  // whether the last MLE launch was k_mle_fused_hw (qt_get_mle_helper_wave)
  // The shape the specialised kernels are compiled for (qt::SpecArgs): three two-outcome settings per qubit (R1 = 6,
  // K = d, M = 6^n <= 4 G and the segmented shots check), both tables paired and their stages on, equal shots, the
  // shots check on.  Everything else -- 'sic', 'proj4', 'proj', unequal shots, plain arrays -- takes the generic body.
  bool spec_eligible() const {
    return mle_specialise && nq <= 3 && povm.registered && povm.prod.enabled && povm.prod.R1 == 6 && K == d &&
           paired_stages && povm.paired_tables == 3 && povm.image_ready && povm.prod.uniform && check_shots;
  }
  qt::SpecArgs spec_args(int extra) const {
    qt::SpecArgs a{povm.image.p, povm.Ns.as<double>(), povm.ns_tot, povm.prod.wuni, jtol2, M, extra, {}, {}};
    for (int k = 0; k < 12; ++k) {
      a.cT[k] = povm.prod.cT[k];
      a.cP[k] = povm.prod.cP[k];
    }
    return a;
  }
  // the POVM as the estimator kernels read it; `extra` (PovmView::extra) comes with the launch's LDS size (Plan)
  qt::PovmView view(int extra) const {
    qt::PovmView v{povm.Aw.as<double>(), povm.AwT.as<double>(), povm.PinvT.as<double>(), M, povm.prod, jtol2,
                   check_shots ? povm.Ns.as<double>() : nullptr, S, K, povm.ns_tot, extra};
    v.pr.pairedT = paired_stages ? povm.paired_tables & 1 : 0;
    v.pr.pairedP = paired_stages ? (povm.paired_tables >> 1) & 1 : 0;
    return v;
  }
  // Jacobi stopping rule off^2 <= jtol2 * ||A||_F^2.  Measured on the C2 batch: the last sweep takes off^2
  // from > 1e-9 to < 1e-28 in one go, so no looser threshold saves a sweep without costing accuracy.
  double jtol2 = 1e-28;
  // qt_states_choi_batch, one slice: the test's flags, the failing trials' places (fail[nb + 1], its exclusive sum pos[nb + 1],
  // the scan's temporary storage), their matrices before and after the projection with its iteration counts, and the
  // slice's Choi matrices when the caller of qt_states_choi_dist_group_batch wants only the distances
  DevBuf sc_ok, sc_fail, sc_pos, sc_tmp, sc_in, sc_out, sc_iters, sc_choi;
};

namespace {

// Every entry point runs on the handle's device and leaves the calling thread's current device as it found
// it: a caller that shares the process with PyTorch (one rank per GPU) must not see torch's current device
// move because an engine call happened to target another card.
struct DeviceScope {
  int prev = -1, want = -1;
  hipError_t err = hipSuccess;
  explicit DeviceScope(int device) : want(device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != want) err = hipSetDevice(want);
  }
  ~DeviceScope() {
    if (prev >= 0 && prev != want) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

#define QT_ENTER(h)                                                                                          \
  if (!(h)) return fail(QT_ERR_ARG, "null handle");                                                          \
  DeviceScope qt_scope_((h)->device);                                                                        \
  if (qt_scope_.err != hipSuccess) return fail(QT_ERR_HIP, "hipSetDevice(%d): %s", (h)->device, hipGetErrorString(qt_scope_.err)); \
  (h)->mail_used = 0

inline int grid_for(size_t total, int block = 256, int cap = 8192) {
  size_t g = (total + block - 1) / block;
  if (g < 1) g = 1;
  if (g > (size_t)cap) g = cap;
  return (int)g;
}

constexpr size_t kMailCap = 1 << 20, kMailMax = 128 << 10;
inline char* mail_alloc(qt_handle_t* h, size_t bytes) {
  if (bytes == 0 || bytes > kMailMax) return nullptr;
  if (!h->mail && hipHostMalloc(reinterpret_cast<void**>(&h->mail), kMailCap, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    h->mail = nullptr;
    return nullptr;
  }
  const size_t at = (h->mail_used + 63) & ~(size_t)63;
  if (at + bytes > kMailCap) return nullptr;
  h->mail_used = at + bytes;
  return h->mail + at;
}
// Wait for the handle's stream.  hipStreamSynchronize / hipEventSynchronize park the thread and wake it through an
// interrupt: ~50 us of latency measured around a 330 us timed region (20 steps of bench.py) and on every host-pointer
// call.  Most waits here are shorter than a millisecond, so: record an event, poll it for up to ~2 ms, then block.
int wait_event_spin(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipEventQuery(ev);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(QT_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(q));
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
  HIPCHK(hipEventSynchronize(ev));
  return 0;
}
int wait_stream(qt_handle_t* h) {
  // poll the stream itself (no event packet to push through the queue first: an idle wait costs ~2 us instead of ~12)
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipStreamQuery(h->stream);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(QT_ERR_HIP, "hipStreamQuery: %s", hipGetErrorString(q));
    if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

// The host-pointer / device-pointer convention of the C ABI, one object per entry point that takes or returns the
// caller's arrays.  With QT_DEVICE_PTR the arrays are device memory and pass straight through: nothing is recorded and
// done() costs one hipGetLastError.  Otherwise every array gets a staging buffer of its own (h->stage[], in the order
// the call registers them), small inputs go through the pinned mailbox, and done() copies the outputs back after the
// launches, in registration order.  Those copy-backs live in the Call: a call that returns early with an error drops
// them, so they never reach arrays its caller may already have freed.
class Call {
 public:
  // `fn` (the calling entry point, by default) names the call in errors
  Call(qt_handle_t* h, int flags, const char* fn = __builtin_FUNCTION())
      : h_(h), fn_(fn), dev_((flags & QT_DEVICE_PTR) != 0) {}
  bool device() const { return dev_; }
  // direction of a copy from device memory to the caller's array
  hipMemcpyKind to_caller() const { return dev_ ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }

  // Input array: the caller's device pointer, or a staged copy of its host array.  A null or empty array passes through.
  template <class T>
  int in(const T* src, size_t count, const T** dev) {
    *dev = src;
    if (dev_ || !src || count == 0) return 0;
    DevBuf* buf;
    if (int r = next(&buf, count * sizeof(T))) return r;
    const void* from = src;
    if (char* m = mail_alloc(h_, count * sizeof(T))) {
      memcpy(m, src, count * sizeof(T));
      from = m;
    }
    HIPCHK(hipMemcpyAsync(buf->p, from, count * sizeof(T), hipMemcpyHostToDevice, h_->stream));
    *dev = buf->as<T>();
    return 0;
  }
  // Output array (null: not wanted, *dev = null): the caller's device pointer, or a buffer that done() copies back.
  template <class T>
  int out(T* dst, size_t count, T** dev) {
    *dev = dst;
    if (dev_ || !dst) return 0;
    DevBuf* buf;
    if (int r = next(&buf, count * sizeof(T))) return r;
    *dev = buf->as<T>();
    back_[nback_++] = {dst, buf->p, count * sizeof(T), nullptr};
    return 0;
  }
  // Array updated in place: staged in like an input, copied back like an output.
  template <class T>
  int inout(T* x, size_t count, T** dev) {
    const T* d;
    if (int r = in(static_cast<const T*>(x), count, &d)) return r;
    *dev = const_cast<T*>(d);
    if (d != x) back_[nback_++] = {x, d, count * sizeof(T), nullptr};
    return 0;
  }
  // The caller's array from / to device memory the handle owns: one direct copy, enqueued now (a null dst: none).
  template <class T>
  int copy_in(T* resident, const T* src, size_t count) {
    HIPCHK(hipMemcpyAsync(resident, src, count * sizeof(T), dev_ ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          h_->stream));
    return 0;
  }
  template <class T>
  int copy_out(T* dst, const T* resident, size_t count) {
    if (dst) HIPCHK(hipMemcpyAsync(dst, resident, count * sizeof(T), to_caller(), h_->stream));
    return 0;
  }
  // The caller's array into a host vector, synchronously.
  template <class T>
  int read(std::vector<T>& v, const T* src, size_t count) {
    v.resize(count);
    if (dev_) HIPCHK(hipMemcpy(v.data(), src, count * sizeof(T), hipMemcpyDeviceToHost));
    else memcpy(v.data(), src, count * sizeof(T));
    return 0;
  }

  // End of the call: enqueue the copy-backs, check the launches, and with host arrays wait for the stream and hand the
  // outputs parked in the mailbox over.  Returns the number of non-zero entries of status[B] (host arrays; 0 otherwise).
  int done(const int32_t* status = nullptr, int B = 0) {
    for (int k = 0; k < nback_; ++k) {
      Back& o = back_[k];
      o.mail = mail_alloc(h_, o.bytes);
      HIPCHK(hipMemcpyAsync(o.mail ? o.mail : o.dst, o.dev, o.bytes, hipMemcpyDeviceToHost, h_->stream));
    }
    HIPCHK(hipGetLastError());
    if (dev_) return 0;
    if (int r = wait_stream(h_)) return r;
    for (int k = 0; k < nback_; ++k)
      if (back_[k].mail) memcpy(back_[k].dst, back_[k].mail, back_[k].bytes);
    int bad = 0;
    if (status)
      for (int b = 0; b < B; ++b) bad += status[b] != 0;
    return bad;
  }

 private:
  struct Back {  // a pending copy-back: dev -> (mail ->) dst
    void* dst;
    const void* dev;
    size_t bytes;
    char* mail;
  };
  int next(DevBuf** buf, size_t bytes) {
    if (nbuf_ == kStageBufs) return fail(QT_ERR_ARG, "%s: more than %d staged arrays", fn_, kStageBufs);
    *buf = &h_->stage[nbuf_++];
    HIPCHK((*buf)->ensure(bytes));
    return 0;
  }
  qt_handle_t* h_;
  const char* fn_;
  bool dev_;
  int nbuf_ = 0, nback_ = 0;
  Back back_[kStageBufs];  // at most one per staging buffer
};

constexpr size_t kLdsLimit = 160 * 1024;  // LDS per CU on gfx950; one workgroup may use all of it

// Launch `kernel` on the handle's stream with `lds` bytes of dynamic LDS.  More than a CU has is refused; above the 64 KB
// default the kernel's attribute is raised first.
template <class... P, class... A>
int launch(qt_handle_t* h, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, A... args) {
  if (lds > kLdsLimit) return fail(QT_ERR_UNSUPPORTED, "launch needs %zu B of LDS per workgroup (more than a CU has)", lds);
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      (void)hipGetLastError();  // reported here: the next hipGetLastError() check, on any handle, must not find it
      return fail(QT_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu): %s", lds, hipGetErrorString(e));
    }
  }
  kernel<<<grid, block, lds, h->stream>>>(args...);
  return 0;
}

// One launch of an estimator kernel (qt_small.h, qt_large.h): its geometry, its dynamic LDS, and the PovmView whose
// `extra` field describes that LDS to the kernel.
struct Plan {
  dim3 grid, block;
  size_t lds;
  qt::PovmView pv;
};
template <class... P, class... A>
int launch(qt_handle_t* h, void (*kernel)(P...), const Plan& p, A... args) {
  return launch(h, kernel, p.grid, p.block, p.lds, args...);
}

// n = 1..3, B trials: Small<NQ>::TPB of them per workgroup, each with the scratch for an M-row POVM and `extra` doubles
// behind it (PovmView::extra: k_mle_bfgs / k_mle_fused), and the tables of an R1-row one-qubit factor once per workgroup.
// (These kernels stream their dense operand from L2 -- dot_global -- and hold no POVM in LDS.)
template <int NQ>
Plan small_plan(const qt_handle_t* h, int B, int M, int R1, int extra) {
  using S = qt::Small<NQ>;
  return {dim3((B + S::TPB - 1) / S::TPB), dim3(S::NT), S::lds_bytes(M, R1, extra), h->view(extra)};
}

// n = 4, 5, B trials, one per workgroup: LDS for an M-row POVM with an R1-row one-qubit factor and `max_iter` BFGS
// iterations of two-loop scalars.  At n = 5 a 32-bit copy of the trial's counts in R-order (Large::make_ctx) goes behind
// all that, PovmView::extra giving its offset in doubles, whenever it fits and the registered shots fit 32 bits.  (n = 4:
// measured slower with the cache, 0.122 vs 0.101 ms per 1024 'mle'.)
template <int NQ>
Plan large_plan(const qt_handle_t* h, int B, int M, int R1, int max_iter) {
  size_t lds = qt::Large<NQ>::lds_bytes(M, R1, max_iter);
  int extra = 0;
  const size_t cache = 4 * (size_t)M + 8;
  if (NQ == 5 && h->povm.prod.enabled && h->povm.ns_max < 4294967296.0 && lds + cache <= kLdsLimit) {
    extra = (int)(lds / 8);
    lds += cache;
  }
  return {dim3(B), dim3(qt::Large<NQ>::NT), lds, h->view(extra)};
}

// An estimator over the handle's POVM.  `extra`: doubles per trial behind the scratch at n <= 3, BFGS iterations at n >= 4.
template <int NQ>
Plan povm_plan(const qt_handle_t* h, int B, int extra = 0) {
  if constexpr (NQ <= 3) return small_plan<NQ>(h, B, h->M, h->povm.prod.enabled ? h->povm.prod.R1 : 0, extra);
  else return large_plan<NQ>(h, B, h->M, h->povm.prod.R1, extra);
}

// The Cholesky parametrisation, which reads no POVM: scratch only, and an empty PovmView.
template <int NQ>
Plan chol_plan(const qt_handle_t* h, int B) {
  Plan p;
  if constexpr (NQ <= 3) p = small_plan<NQ>(h, B, 0, 0, 0);
  else p = large_plan<NQ>(h, B, 0, 1, 0);
  p.pv = qt::PovmView{};
  return p;
}

// f(std::integral_constant<int, n>()) for the handle's n: the kernels of qt_small.h (n <= 3) and qt_large.h (n = 4, 5)
// are templates on it.
template <class F>
int by_nq(const qt_handle_t* h, F f) {
  switch (h->nq) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    default: return fail(QT_ERR_UNSUPPORTED, "n_qubits %d", h->nq);
  }
}

// In-place inverse of the n x n matrix in the left half of aug [n][2n]: one workgroup up to n = 127, the
// chip-wide variant (qt_ops.h) beyond -- the 256 x 256 complex Gram matrix of 2-qubit process tomography takes
// 12.5 ms in one workgroup and 1.8 ms as 2 x 256 small launches.
template <int CPLX>
int launch_gauss_jordan(qt_handle_t* h, int n, double* aug, int* info) {
  if (n < 128) return launch(h, qt::k_gauss_jordan<CPLX>, dim3(1), dim3(1024), 0, n, aug, info);
  if (int r = launch(h, qt::k_gj_identity<CPLX>, dim3(grid_for((size_t)n * n)), dim3(256), 0, n, aug, info)) return r;
  for (int k = 0; k < n; ++k) {
    if (int r = launch(h, qt::k_gj_pivot<CPLX>, dim3(1), dim3(1024), 0, n, aug, k, info)) return r;
    if (int r = launch(h, qt::k_gj_eliminate<CPLX>, dim3(n), dim3(256), 0, n, aug, k)) return r;
  }
  return 0;
}

template <int W>
int launch_transpose(qt_handle_t* h, const double* in, int R, int C, double* out) {
  constexpr int TS = 64 / W;
  return launch(h, qt::k_transpose_tiled<W>, dim3((C + TS - 1) / TS, (R + TS - 1) / TS), dim3(256), 0, in, R, C, out);
}

// out[cols][rows] = inv(A^T A) A^T of A[rows][cols], real (W = 1) or complex (W = 2; plain transposes, routines.py:69-71):
// Gram GEMM, pivoted Gauss-Jordan in h->aug, GEMM, enqueued on the handle's stream; the pivot report lands in h->info
// (0 = regular).  AT, when given, is A^T [cols][rows], read by the second GEMM in place of A.
template <int W>
int enqueue_left_inverse(qt_handle_t* h, const double* A, int rows, int cols, double* out, const double* AT = nullptr) {
  constexpr int CPLX = W - 1;
  HIPCHK(h->aug.ensure((size_t)cols * 2 * cols * W * sizeof(double)));
  HIPCHK(h->info.ensure(sizeof(int)));
  double* g = h->aug.as<double>();
  if (int r = launch(h, qt::k_gemm<CPLX>, dim3((cols + 15) / 16, (cols + 15) / 16), dim3(64), 0, cols, cols, rows, A, cols, 1,
                     A, cols, 0, g, 2 * cols))
    return r;
  if (int r = launch_gauss_jordan<CPLX>(h, cols, g, h->info.as<int>())) return r;
  return launch(h, qt::k_gemm<CPLX>, dim3((rows + 15) / 16, (cols + 15) / 16), dim3(64), 0, cols, rows, cols,
                g + (size_t)cols * W, 2 * cols, 0, AT ? AT : A, AT ? rows : cols, AT ? 0 : 1, out, rows);
}

int need_povm(qt_handle_t* h) {
  if (!h->povm.registered) return fail(QT_ERR_STATE, "qt_set_povm has not been called on this handle");
  return 0;
}

// Row digits for k_povm_kron: row = s K + k with s = sum_q s_q S1^(n-1-q), k likewise; byte q = s_q K1 + k_q.
int ensure_kron_digits(qt_handle_t* h, int S1, int K1) {
  if (h->kron_S1 == S1 && h->kron_K1 == K1 && h->kron_dig.p) return 0;
  const int n = h->nq;
  long long S = 1, K = 1;
  for (int q = 0; q < n; ++q) {
    S *= S1;
    K *= K1;
  }
  std::vector<unsigned long long> dig((size_t)(S * K));
  for (long long s = 0; s < S; ++s)
    for (long long k = 0; k < K; ++k) {
      unsigned long long pack = 0;
      long long sr = s, kr = k;
      for (int q = n - 1; q >= 0; --q) {
        pack |= (unsigned long long)((sr % S1) * K1 + (kr % K1)) << (8 * q);
        sr /= S1;
        kr /= K1;
      }
      dig[(size_t)(s * K + k)] = pack;
    }
  h->kron_S1 = h->kron_K1 = 0;
  HIPCHK(h->kron_dig.ensure(dig.size() * sizeof(unsigned long long)));
  HIPCHK(hipMemcpyAsync(h->kron_dig.p, dig.data(), dig.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));  // `dig` goes out of scope
  h->kron_S1 = S1;
  h->kron_K1 = K1;
  return 0;
}

int launch_povm_kron(qt_handle_t* h, const double* dtable, int S1, int K1, double* dout) {
  if (S1 * K1 > 255) return fail(QT_ERR_UNSUPPORTED, "one-qubit table with %d rows (> 255)", S1 * K1);
  if (int r = ensure_kron_digits(h, S1, K1)) return r;
  size_t total = (size_t)h->D;
  for (int q = 0; q < h->nq; ++q) total *= (size_t)S1 * K1;
  if ((total >> (2 * h->nq)) > ((size_t)1 << 31)) return fail(QT_ERR_UNSUPPORTED, "POVM tensor too large");
  // >> 256 workgroups, each lane a 16-byte store per pass
  return launch(h, qt::k_povm_kron, dim3(grid_for(total / 2, 256, 4096)), dim3(256), 0, h->nq, dtable, S1 * K1,
                h->kron_dig.as<unsigned long long>(), total, dout);
}

// Dense operands A ([M][D]; the Kronecker power of the table for a product POVM), A^T, A', A'^T -- built when first
// needed: Born kernel / dense estimators at n <= 3, process set-up, the dense left inverse.
int ensure_dense(qt_handle_t* h) {
  PovmState& pm = h->povm;
  if (pm.dense_ready) return 0;
  const size_t bytes = (size_t)h->M * h->D * sizeof(double);
  HIPCHK(pm.A.ensure(bytes));
  HIPCHK(pm.AT.ensure(bytes));
  HIPCHK(pm.Aw.ensure(bytes));
  HIPCHK(pm.AwT.ensure(bytes));
  if (!pm.a_loaded) {
    if (pm.S1 * pm.K1 == 0) return fail(QT_ERR_STATE, "no POVM tensor to build the dense operands from");
    if (int r = launch_povm_kron(h, pm.T.as<double>(), pm.S1, pm.K1, pm.A.as<double>())) return r;
    pm.a_loaded = true;
  }
  if (int r = launch(h, qt::k_povm_setup, dim3((h->D + 63) / 64, (h->M + 63) / 64), dim3(256), 0, pm.A.as<double>(),
                     pm.Ns.as<double>(), pm.ns_tot, h->K, h->M, h->D, pm.AT.as<double>(), pm.Aw.as<double>(), pm.AwT.as<double>()))
    return r;
  HIPCHK(hipGetLastError());
  pm.dense_ready = true;
  return 0;
}

// Dense left inverse inv(A'^T A') A'^T of the cached weighted POVM.
int compute_dense_pinv(qt_handle_t* h) {
  if (int r = ensure_dense(h)) return r;
  PovmState& pm = h->povm;
  const int D = h->D, M = h->M;
  const size_t bytes = (size_t)M * D * sizeof(double);
  HIPCHK(pm.Pinv.ensure(bytes));
  HIPCHK(pm.PinvT.ensure(bytes));
  if (int r = enqueue_left_inverse<1>(h, pm.Aw.as<double>(), M, D, pm.Pinv.as<double>(), pm.AwT.as<double>())) return r;
  if (int r = launch_transpose<1>(h, pm.Pinv.as<double>(), D, M, pm.PinvT.as<double>())) return r;
  int info = 0;
  HIPCHK(hipMemcpyAsync(&info, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  if (info != 0) return fail(QT_ERR_SINGULAR, "A^T A is singular (no pivot in column %d): POVM not informationally complete", info - 1);
  pm.pinv_ready = true;
  return 0;
}

// n >= 4: what the launch about to be made reads besides the factorised tables.  A plain tensor (qt_set_povm) has its
// dense operands and left inverse already; a product POVM with unequal shots needs the dense left inverse for 'lin'.
int prepare_large(qt_handle_t* h, bool needs_lin) {
  if (h->povm.prod.enabled && needs_lin && !h->povm.prod.uniform && !h->povm.pinv_ready) return compute_dense_pinv(h);
  return 0;
}

// Start of qt_set_povm / qt_set_povm_product: forget the previous POVM and the process set-up on top of it, record the
// shape.  (The device memory of both stays, for reuse.)
int begin_povm(qt_handle_t* h, int S, int K) {
  const size_t M = (size_t)S * K;
  if (M < (size_t)h->D) return fail(QT_ERR_SINGULAR, "POVM has %zu rows < D = %d: not informationally complete", M, h->D);
  h->povm.reset();
  h->proc_set = false;
  h->S = S;
  h->K = K;
  h->M = (int)M;
  HIPCHK(h->povm.Ns.ensure(S * sizeof(double)));
  HIPCHK(h->info.ensure(sizeof(int)));
  return 0;
}

// buf = v, enqueued on the handle's stream: `v` must outlive the copy
template <class T>
int upload(qt_handle_t* h, DevBuf& buf, const std::vector<T>& v) {
  if (v.empty()) return 0;
  HIPCHK(buf.ensure(v.size() * sizeof(T)));
  HIPCHK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return 0;
}

int check_pvals(int period, int K, const int64_t* n, const double* pvals) {
  for (int s = 0; s < period; ++s) {
    if (n[s] < 0) return fail(QT_ERR_ARG, "n < 0 in row %d", s);
    // RandomState.multinomial's own checks (mtrand.pyx): every pval in [0, 1], and the leading K - 1 may not exceed 1
    double head = 0.0, comp = 0.0;  // compensated sum, as NumPy's check has it
    for (int j = 0; j < K; ++j) {
      const double p = pvals[(size_t)s * K + j];
      if (!(p >= 0.0 && p <= 1.0)) return fail(QT_ERR_ARG, "pvals < 0, pvals > 1 or pvals contains NaNs");
      if (j == 0 && K > 1) head = p;
      if (j > 0 && j < K - 1) {
        const double y = p - comp, t = head + y;
        comp = (t - head) - y;
        head = t;
      }
    }
    if (head > 1.0 + 1e-12) return fail(QT_ERR_ARG, "sum(pvals[:-1]) > 1.0");
  }
  return 0;
}

// a6 + a7 (+ a16 when `dist` is asked for): one body behind qt_lin_batch, qt_lin_dist_batch and qt_lin_dist_group_batch.
// `centre` holds G matrices; trial b is measured against centre b % G (qt::EstOut).
int lin_batch_impl(qt_handle_t* h, const int64_t* counts, int B, int physical, const double* centre, int G, double* rho,
                   double* dist, double* bloch_out, int32_t* status, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (B < 0 || G < 1 || (B > 0 && (!counts || (!rho && !dist) || (dist && !centre)))) return fail(QT_ERR_ARG, "bad lin_batch arguments");
  if (B == 0) return 0;
  const int64_t* dc;
  const double* dcen;
  double *drho, *dbl, *ddist;
  int32_t* dst;
  const size_t nel = (size_t)B * h->D;
  if (int r = c.in(counts, (size_t)B * h->M, &dc)) return r;
  if (int r = c.in(centre, (size_t)G * h->D * 2, &dcen)) return r;
  if (int r = c.out(rho, nel * 2, &drho)) return r;
  if (int r = c.out(bloch_out, nel, &dbl)) return r;
  if (int r = c.out(status, (size_t)B, &dst)) return r;
  if (int r = c.out(dist, (size_t)B, &ddist)) return r;
  const qt::EstOut eo{drho, dcen, ddist, G, 0};
  if (h->nq >= 4)
    if (int r = prepare_large(h, true)) return r;
  if (int r = by_nq(h, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const Plan p = povm_plan<NQ>(h, B);
        if constexpr (NQ <= 3) return launch(h, qt::k_lin_batch<NQ>, p, p.pv, dc, B, physical, eo, dbl, dst);
        else return launch(h, qt::k_lin_large<NQ>, p, p.pv, dc, B, physical, eo, dbl, dst);
      }))
    return r;
  return c.done(status, B);
}

// The per-trial arrays of an MLE batch; at(b0): those of the trials from b0 on (a null output stays null).
struct MleArrays {
  const int64_t* counts;
  qt::EstOut eo;
  int32_t *nit, *nfev;
  double* fun;
  int32_t* status;
  double *x, *g, *f;  // the hand-off from k_mle_*start to k_mle_*bfgs
  int32_t* act;
  int M, D;
  MleArrays at(int b0) const {
    auto off = [b0](auto* p, size_t per) { return p ? p + (size_t)b0 * per : p; };
    return {off(counts, M), {off(eo.rho, 2 * D), eo.centre, off(eo.dist, 1), eo.G, (int)((eo.g0 + (long long)b0) % eo.G)},
            off(nit, 1), off(nfev, 1), off(fun, 1),
            off(status, 1), off(x, D), off(g, D), off(f, 1), off(act, 1), M, D};
  }
};

// The split MLE pair: k_mle_start / k_mle_bfgs (qt_mle_small.h) at n <= 3, k_mle_large_start / k_mle_large_bfgs (qt_large.h)
// at n = 4, 5.
template <int NQ, bool GENERIC>
auto mle_split_kernels() {
  if constexpr (NQ <= 3) return std::make_pair(qt::k_mle_start<NQ, GENERIC>, qt::k_mle_bfgs<NQ, GENERIC>);
  else return std::make_pair(qt::k_mle_large_start<NQ>, qt::k_mle_large_bfgs<NQ>);
}
// The POVM argument of an n <= 3 MLE kernel: the PovmView of the plan, or the slim struct of the specialised instantiation.
template <bool GENERIC>
auto mle_povm_arg(const qt_handle_t* h, const Plan& p) {
  if constexpr (GENERIC) return p.pv;
  else return h->spec_args(p.pv.extra);
}
// One launch of an n <= 3 MLE kernel: the leading plain arguments (qt_args.h: mle_front) taken off the POVM struct that
// follows them, then `rest`.  The generic kernels have no table image: nullptr.
template <bool GENERIC, class K, class... R>
int launch_mle(qt_handle_t* h, K kernel, const Plan& p, const int64_t* counts, int B, int max_iter, double tol, R... rest) {
  const auto pv = mle_povm_arg<GENERIC>(h, p);
  const void* image = nullptr;
  if constexpr (!GENERIC) image = pv.image;
  return launch(h, kernel, p, counts, image, pv.Ns, B, pv.M, pv.extra, max_iter, tol, pv, rest...);
}

// The largest max_iter whose BFGS launch of the split pair (povm_plan<NQ>(h, ., extra) in mle_batch_impl: 2 doubles per
// iteration and trial behind the scratch, at n = 3 for each of a workgroup's TPB trials and behind the parked
// line-search state) fits a CU's LDS with the handle's POVM -- beside the LDS that the compiled kernel holds by itself
// (k_mle_bfgs<3, .>: 256 B), which the dynamic part cannot use.  `spec`: the specialised instantiation runs (n = 3).
template <int NQ>
int mle_iter_cap(const qt_handle_t* h, bool spec, int* cap) {
  size_t base, per_iter;
  const void* kernel;
  if constexpr (NQ == 3) {
    base = qt::Small<3>::lds_bytes(h->M, h->povm.prod.enabled ? h->povm.prod.R1 : 0, qt::LineSearch::SLOTS);
    per_iter = (size_t)qt::Small<3>::TPB * 2 * sizeof(double);
    kernel = spec ? reinterpret_cast<const void*>(mle_split_kernels<3, false>().second)
                  : reinterpret_cast<const void*>(mle_split_kernels<3, true>().second);
  } else {
    base = qt::Large<NQ>::lds_bytes(h->M, h->povm.prod.R1, 0);
    per_iter = 2 * sizeof(double);
    kernel = reinterpret_cast<const void*>(mle_split_kernels<NQ, true>().second);
  }
  hipFuncAttributes attr;
  HIPCHK(hipFuncGetAttributes(&attr, kernel));
  base += attr.sharedSizeBytes;
  *cap = base > kLdsLimit ? 0 : (int)((kLdsLimit - base) / per_iter);
  return 0;
}

// a8-a10 (+ a16 when `dist` is asked for): one body behind qt_mle_batch, qt_mle_dist_batch and qt_mle_dist_group_batch.
// `centre` holds G matrices; trial b is measured against centre b % G (qt::EstOut).
int mle_batch_impl(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol, const double* centre, int G,
                   double* rho, double* dist, int32_t* nit, int32_t* nfev, double* fun, int32_t* status, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (B < 0 || G < 1 || (B > 0 && (!counts || (!rho && !dist) || (dist && !centre)))) return fail(QT_ERR_ARG, "bad mle_batch arguments");
  if (init != QT_INIT_LIN && init != QT_INIT_MIXED) return fail(QT_ERR_ARG, "init must be QT_INIT_LIN or QT_INIT_MIXED");
  if (max_iter < 0) return fail(QT_ERR_ARG, "max_iter < 0");
  if (B == 0) return 0;
  const int64_t* dc;
  const double* dcen;
  double *drho, *dfun, *ddist;
  int32_t *dnit, *dnfev, *dst;
  const size_t nel = (size_t)B * h->D;
  if (int r = c.in(counts, (size_t)B * h->M, &dc)) return r;
  if (int r = c.in(centre, (size_t)G * h->D * 2, &dcen)) return r;
  if (int r = c.out(rho, nel * 2, &drho)) return r;
  if (int r = c.out(nit, (size_t)B, &dnit)) return r;
  if (int r = c.out(nfev, (size_t)B, &dnfev)) return r;
  if (int r = c.out(fun, (size_t)B, &dfun)) return r;
  if (int r = c.out(status, (size_t)B, &dst)) return r;
  if (int r = c.out(dist, (size_t)B, &ddist)) return r;
  const qt::EstOut eo{drho, dcen, ddist, G, 0};
  // n >= 3 keeps rho_i / alpha_i of every BFGS iteration in the trial's LDS (16 bytes per iteration and trial): at most
  // 4096 iterations at n = 4, 5 and 2000 at n = 3 (the one-launch kernel, which also keeps 24 pairs there, up to 256 of
  // them), and no more than fit a CU's LDS beside this POVM's scratch (mle_iter_cap) -- refused here, before any launch.
  // (Up to 256 iterations the cap is not worked out: what does not fit then is refused by launch().)
  h->last_mle_spec = h->spec_eligible();
  h->last_mle_helper = false;
  if (h->nq >= 3) {
    const int ceiling = h->nq == 3 ? 2000 : 4096;
    if (max_iter > ceiling)
      return fail(QT_ERR_UNSUPPORTED, "max_iter > %d is not supported for n_qubits = %d (LDS holds the two-loop scalars)", ceiling, h->nq);
    if (max_iter > 256) {
      int cap = 0;
      if (int r = by_nq(h, [&](auto nq) -> int {
            constexpr int NQ = decltype(nq)::value;
            if constexpr (NQ >= 3) return mle_iter_cap<NQ>(h, h->last_mle_spec, &cap);
            else return 0;
          }))
        return r;
      if (max_iter > cap)
        return fail(QT_ERR_UNSUPPORTED, "max_iter = %d is not supported for this POVM at n_qubits = %d: beside its %d rows a CU's "
                    "LDS holds the two-loop scalars of at most %d iterations", max_iter, h->nq, h->M, cap);
    }
  }
  if (h->nq >= 4)
    if (int r = prepare_large(h, init == QT_INIT_LIN)) return r;
  const int mi = max_iter > 0 ? max_iter : 1;
  return by_nq(h, [&](auto nq) -> int {
    constexpr int NQ = decltype(nq)::value;
    if constexpr (NQ <= 3) {
      // up to one resident wave per SIMD (1024 trial-waves) the single fused launch wins; beyond that the
      // 256-VGPR BFGS loop would cap occupancy for every trial, so the split pair is used
      constexpr int TPW = qt::Small<NQ>::TPW;
      if ((B + TPW - 1) / TPW <= h->fused_max_waves && !(NQ == 3 && max_iter > 256)) {
        int extra = 0;
        bool helper = false;
        size_t lds_hw = 0;  // k_mle_fused_hw's dynamic LDS: computed once, for the fit check and for the launch
        if (NQ == 3) {  // two-loop BFGS: line-search state, rho_i, alpha_i and the first pairs in LDS, later pairs in global
          const int state = qt::LineSearch::SLOTS + 2 * mi;
          // k_mle_fused_hw (the generic body meets its twins at the barrier behind the product POVM's tables) keeps fewer
          // pairs in LDS and a scratch per twin wavefront behind the trials'; where that does not fit, k_mle_fused runs
          const int extra_hw = state + qt::kFusedHwLdsPairs * 2 * h->D;
          lds_hw = qt::Small<3>::lds_bytes_twin(h->M, h->povm.prod.R1, extra_hw);
          helper = h->mle_helper_wave && init == QT_INIT_LIN && h->povm.prod.enabled && lds_hw <= kLdsLimit;
          const int lds_pairs = helper ? qt::kFusedHwLdsPairs : qt::kFusedLdsPairs;
          extra = state + lds_pairs * 2 * h->D;
          const int over = mi > lds_pairs ? mi : 1;  // (indexed by pair number: rows below lds_pairs stay unused)
          HIPCHK(h->hess.ensure((size_t)B * over * 2 * h->D * sizeof(double)));
        }
        Plan p = povm_plan<NQ>(h, B, extra);
        auto fused = [&](auto generic) {
          constexpr bool GEN = decltype(generic)::value;
          if constexpr (NQ == 3) {
            if (helper) {
              h->last_mle_helper = true;
              p.block = dim3(qt::Small<NQ>::NT, 2);  // y = 1: the twin wavefronts
              p.lds = lds_hw;
              return launch_mle<GEN>(h, qt::k_mle_fused_hw<NQ, GEN>, p, dc, B, max_iter, tol, eo, dnit, dnfev, dfun, dst,
                                     h->hess.as<double>());
            }
          }
          return launch_mle<GEN>(h, init == QT_INIT_LIN ? qt::k_mle_fused<NQ, GEN> : qt::k_mle_fused_mixed<NQ, GEN>, p, dc, B,
                                 max_iter, tol, eo, dnit, dnfev, dfun, dst, h->hess.as<double>());
        };
        if (int r = h->last_mle_spec ? fused(std::false_type()) : fused(std::true_type())) return r;
        return c.done(status, B);
      }
    }
    HIPCHK(h->ws_x.ensure(nel * sizeof(double)));
    HIPCHK(h->ws_g.ensure(nel * sizeof(double)));
    HIPCHK(h->ws_f.ensure((size_t)B * sizeof(double)));
    HIPCHK(h->ws_act.ensure((size_t)B * sizeof(int32_t)));
    // BFGS history of the trials that iterate: 2 D doubles per iteration and trial (two-loop recursion), in chunks of
    // <= 4 GiB.  (n = 1, 2 keep the 4 / 16-entry Hessian rows in registers: no workspace.)
    int chunk = B;
    if (NQ >= 3) {
      const size_t per_trial = (size_t)mi * 2 * h->D * sizeof(double);
      chunk = (int)(((size_t)4 << 30) / per_trial);
      if (chunk < 1) chunk = 1;
      if (chunk > B) chunk = B;
      HIPCHK(h->hess.ensure((size_t)chunk * per_trial));
    }
    const MleArrays all{dc, eo, dnit, dnfev, dfun, dst, h->ws_x.as<double>(), h->ws_g.as<double>(), h->ws_f.as<double>(),
                        h->ws_act.as<int32_t>(), h->M, h->D};
    // start point + first evaluation of every trial; then the BFGS loop of those that iterate, chunk by chunk, with
    // rho_i, alpha_i (and at n = 3 the parked line-search state) in LDS
    auto split = [&](auto generic) -> int {
      constexpr bool GEN = decltype(generic)::value || NQ >= 4;
      const auto [k_start, k_bfgs] = mle_split_kernels<NQ, GEN>();
      const Plan ps = povm_plan<NQ>(h, B);
      int r;
      if constexpr (NQ <= 3)
        r = launch_mle<GEN>(h, k_start, ps, dc, B, max_iter, tol, init, eo, dnit, dnfev, dfun, dst, all.x, all.g, all.f, all.act);
      else
        r = launch(h, k_start, ps, ps.pv, dc, B, init, max_iter, tol, eo, dnit, dnfev, dfun, dst, all.x, all.g, all.f, all.act);
      if (r) return r;
      const int extra = NQ >= 4 ? max_iter : (NQ == 3 ? qt::LineSearch::SLOTS + 2 * mi : 0);
      for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        const MleArrays a = all.at(b0);
        const Plan p = povm_plan<NQ>(h, nb, extra);
        if constexpr (NQ <= 3)
          r = launch_mle<GEN>(h, k_bfgs, p, a.counts, nb, max_iter, tol, a.eo, a.nit, a.nfev, a.fun, a.status, a.x, a.g, a.f,
                              a.act, h->hess.as<double>());
        else
          r = launch(h, k_bfgs, p, p.pv, a.counts, nb, max_iter, tol, a.eo, a.nit, a.nfev, a.fun, a.status, a.x, a.g, a.f,
                     a.act, h->hess.as<double>());
        if (r) return r;
      }
      return c.done(status, B);
    };
    return h->last_mle_spec ? split(std::false_type()) : split(std::true_type());
  });
}

// The projection (mode 0: CPTP by Dykstra's alternation, 1: TP, 2: CP) of B Choi matrices by the kernel for the handle's
// size.  n = 3: k_cptp_project64 (qt_process64.h), one workgroup each, with Dykstra's p, q, y, x and the clip's input in
// h->proc_ws -- except in mode 1, which takes no workspace.  n = 2: k_cptp_wave16 (qt_process_wave16.h), one wavefront
// each.  n = 1: k_cptp_project<4> (qt_process.h), one workgroup each.  `iters` and `status` may be null.
// n = 2 only: `dist` (with the table `centres` of G matrices, process b against centre (g0 + b) % G) takes hs_dst(projected
// matrix, centre) from the same launch, and `out` may then be null.
int project(qt_handle_t* h, const double* in, int B, int mode, int n_iter, double tol, double* out, int32_t* iters,
            int32_t* status, const double* centres = nullptr, int G = 1, int g0 = 0, double* dist = nullptr) {
  if (h->D == 64) {
    if (mode != 1) HIPCHK(h->proc_ws.ensure((size_t)B * qt::Proc64::kWsComplex * 2 * sizeof(double)));
    return launch(h, qt::k_cptp_project64, dim3(B), dim3(qt::Proc64::NT), qt::Proc64::kLdsBytes,
                  qt::Cptp64Opts{mode, n_iter, tol}, in, B, out, iters, status, h->proc_ws.as<double>());
  }
  if (h->D == 16)
    return launch(h, qt::k_cptp_wave16, dim3((B + 3) / 4), dim3(256), 0, in, B, mode, n_iter, tol, out, iters, status, centres, G, g0, dist);
  return launch(h, qt::k_cptp_project<4>, dim3(B), dim3(qt::ProcWG<4>::NT), 0, in, B, mode, n_iter, tol, out, iters, status);
}

// The Kronecker factors of the left inverse, L^+ = Pi (V_S^+ (x) V_P^+), from proc.in_states and proc.emats: V_S^+, V_P^+,
// its transpose and, with `groups` > 0, the permuted operand of the matrix-core kernels (k_lifp64: 4 groups, k_lifp16: 1).
// Enqueued on the handle's stream; the two pivot reports are in info[0] (V_S) and info[1] (V_P) once it has been waited for.
int enqueue_factors(qt_handle_t* h, int groups, int info[2]) {
  ProcessState& ps = h->proc;
  const int d = h->d, D = h->D, M = h->M;
  HIPCHK(ps.vs_pinv.ensure((size_t)D * D * 2 * sizeof(double)));
  HIPCHK(ps.vp_pinv.ensure((size_t)D * M * 2 * sizeof(double)));
  HIPCHK(ps.vp_pinvT.ensure((size_t)M * D * 2 * sizeof(double)));
  if (groups) HIPCHK(ps.vp_perm.ensure((size_t)groups * M * 32 * sizeof(double)));
  if (int r = enqueue_left_inverse<2>(h, ps.in_states.as<double>(), D, D, ps.vs_pinv.as<double>())) return r;
  HIPCHK(hipMemcpyAsync(&info[0], h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (int r = enqueue_left_inverse<2>(h, ps.emats.as<double>(), M, D, ps.vp_pinv.as<double>())) return r;
  HIPCHK(hipMemcpyAsync(&info[1], h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (int r = launch_transpose<2>(h, ps.vp_pinv.as<double>(), D, M, ps.vp_pinvT.as<double>())) return r;
  if (groups)
    return launch(h, qt::k_vp_perm, dim3(grid_for((size_t)groups * M * 32)), dim3(256), 0, ps.vp_pinvT.as<double>(), M, D, d,
                  groups, ps.vp_perm.as<double>());
  return 0;
}

// Scratch of the n = 3 'pgdb' iteration over B processes: the per-process workspace (qt::Pgdb64::Ws) in ws_x, the trial
// points c - g / mu in ws_g, their CPTP projections in ws_f, the loop state {iteration, stopped, NaN seen, -} per
// process and the count of running processes in ws_act.
int pgdb64_scratch(qt_handle_t* h, int B) {
  const size_t ne2 = (size_t)h->D * h->D * 2;
  HIPCHK(h->ws_x.ensure((size_t)B * qt::Pgdb64::ws_doubles(h->M) * sizeof(double)));
  HIPCHK(h->ws_g.ensure((size_t)B * ne2 * sizeof(double)));
  HIPCHK(h->ws_f.ensure((size_t)B * ne2 * sizeof(double)));
  HIPCHK(h->ws_act.ensure(((size_t)B * 4 + 4) * sizeof(int32_t)));
  return 0;
}

// The first two launches of an iteration at the points `cur`: model, weights and gradient into the workspace, then the
// projection of the trial points (ws_g -> ws_f).
int pgdb64_trial(qt_handle_t* h, const int64_t* counts, int B, const double* cur) {
  using S = qt::Pgdb64;
  if (int r = launch(h, qt::k_pgdb64_grad, dim3(B), dim3(S::NT), S::kLdsBytes, counts, B, h->M, h->proc.in_states.as<double>(),
                     h->proc.emats.as<double>(), cur, h->ws_act.as<int32_t>(), h->ws_x.as<double>(), h->ws_g.as<double>()))
    return r;
  return project(h, h->ws_g.as<double>(), B, 0, 1000, 1e-12, h->ws_f.as<double>(), nullptr, nullptr);
}

// a5 on device arrays, the launches behind qt_born_probs and qt_process_born_probs: p[B][M] from bloch[B][D]
int born_launch(qt_handle_t* h, const double* din, int B, double* dout) {
  if (h->nq >= 4 && h->povm.prod.enabled) {  // factorised contraction, one workgroup per state
    const Plan pl = h->nq == 4 ? povm_plan<4>(h, B) : povm_plan<5>(h, B);
    return launch(h, h->nq == 4 ? qt::k_born_large<4> : qt::k_born_large<5>, pl, pl.pv, din, B, dout);
  }
  if (int r = ensure_dense(h)) return r;
  const int gx = (h->M + 255) / 256;
  int Mp = (h->M + 15) & ~15;
  if ((Mp & 31) != 16) Mp += 16;  // LDS pitch: 16 mod 32 doubles (see k_born_mfma)
  const size_t at_bytes = (size_t)h->D * Mp * sizeof(double);
  if (h->D <= 64 && at_bytes <= 128 * 1024 && B >= 4096) {
    // batched: the matrix-core kernel, one persistent 16-wave workgroup per CU (A^T lives in its LDS)
    int grid = (B + 16 * 16 - 1) / (16 * 16);
    if (grid > 256) grid = 256;
    const auto kern = h->D == 4 ? qt::k_born_mfma<4> : (h->D == 16 ? qt::k_born_mfma<16> : qt::k_born_mfma<64>);
    return launch(h, kern, dim3(grid), dim3(1024), at_bytes, h->povm.AT.as<double>(), h->M, Mp, h->d, din, B, dout);
  }
  const int TB = h->D <= 256 ? 8 : 4;  // states per workgroup
  int gy = (B + TB - 1) / TB;
  if (gy > 2048) gy = 2048;
  return launch(h, TB == 8 ? qt::k_born<8> : qt::k_born<4>, dim3(gx, gy), dim3(256), TB * h->D * sizeof(double),
                h->povm.AT.as<double>(), h->M, h->D, h->d, din, B, dout);
}

}  // namespace

// ---- qt_polytope_confidence / qt_polytope_coverage: the mapping of a shape, argument checks ---------------------------
namespace {

struct PolyPlan {
  bool wave = false;
  int TS = 0, kshift = 0;  // wave teams
  int NT = 0, mode = 0;    // workgroup per trial
  qt::PolyShape sh{};
  size_t lds = 0;
};

// The mapping is a function of the shape alone.  Workgroup mapping: G = the power of two <= min(K, 64) with the fewest
// serial entries per lane, ceil(R G / NT) rounds of ceil(K / G) entries (the smallest such G).
int poly_plan(int R, int K, PolyPlan* p) {
  const long long RK = (long long)R * K;
  if (RK > INT32_MAX) return fail(QT_ERR_UNSUPPORTED, "polytope kernels index a count table with 32 bits (R K = %lld)", RK);
  const bool pow2 = (K & (K - 1)) == 0;
  p->sh.R = R;
  p->sh.K = K;
  if (RK <= 64 && pow2) {
    p->wave = true;
    p->TS = 8;
    while (p->TS < RK) p->TS *= 2;
    while ((1 << p->kshift) < K) ++p->kshift;
    return 0;
  }
  const size_t lds_f = (size_t)(RK + 16) * sizeof(double);
  p->mode = lds_f <= kLdsLimit ? qt::POLY_LDS : qt::POLY_GLOBAL;
  p->NT = RK <= 1024 ? 64 : RK <= 4096 ? 256 : 1024;
  p->lds = p->mode == qt::POLY_LDS ? lds_f : 16 * sizeof(double);
  long long best = -1;
  for (int G = 1, s = 0; G <= 64 && G <= K; G *= 2, ++s) {
    const long long cost = (((long long)R * G + p->NT - 1) / p->NT) * ((K + G - 1) / G);
    if (best < 0 || cost < best) {
      best = cost;
      p->sh.G = G;
      p->sh.gshift = s;
    }
  }
  return 0;
}

// Every shot number positive and finite, checked on the host before any launch.  Device arrays are read back (R doubles)
// once the handle's stream has finished whatever produces them.
int poly_check_shots(qt_handle_t* h, Call& c, const double* shots, int R, const char* fn) {
  std::vector<double> v;
  if (c.device()) HIPCHK(hipStreamSynchronize(h->stream));
  if (int r = c.read(v, shots, (size_t)R)) return r;
  for (int i = 0; i < R; ++i)
    if (!(v[i] > 0.0) || !std::isfinite(v[i]))
      return fail(QT_ERR_ARG, "%s: shots[%d] = %g is not a positive finite number", fn, i, v[i]);
  return 0;
}

template <class Wave, class Wg>
int poly_dispatch(const PolyPlan& p, Wave wave, Wg wg) {
  if (p.wave) return wave();
  using Lds = std::integral_constant<int, qt::POLY_LDS>;
  if (p.mode == qt::POLY_GLOBAL) return wg(std::integral_constant<int, 1024>{}, std::integral_constant<int, qt::POLY_GLOBAL>{});
  if (p.NT == 64) return wg(std::integral_constant<int, 64>{}, Lds{});
  if (p.NT == 256) return wg(std::integral_constant<int, 256>{}, Lds{});
  return wg(std::integral_constant<int, 1024>{}, Lds{});
}

constexpr long long kPolyMaxGrid = 1 << 20;  // workgroups of the per-trial mapping (each strides over the batch)
// one call: at most 2^31 - 1 workgroups of wave teams (>= 4 pairs each) and counts that a size_t of bytes can hold
constexpr long long kPolyMaxUnits = 1LL << 32, kPolyMaxCounts = 1LL << 44;

}  // namespace

// ---- a11: the Choi linear inversion behind qt_lifp_batch and qt_lifp_dist_batch -----------------------------------
namespace {

// How qt_lifp_batch / qt_lifp_dist_batch reconstruct: chosen once per call from the WHOLE batch, so that the slices of
// a call all take the path (and give the bits) of the unsliced one.
enum LifpPath { kLifp64, kKronGemm, kLifp16, kDenseGemm, kFused };

int lifp_path(qt_handle_t* h, int B, LifpPath* path) {
  const ProcessState& ps = h->proc;
  const int D = h->D, M = h->M;
  const int R = D * M, Rp = ps.factored ? R : (R + 63) / 64 * 64;
  const size_t gemm_lds = ((size_t)Rp * 16 + 4 * 256) * sizeof(double);
  if (ps.factored) {  // n = 3: X = V_S^+ F V_P^+^T, two small products per process (qt_process64.h)
    if ((size_t)B * D > (size_t)1 << 26) return fail(QT_ERR_ARG, "batch too large");
    *path = ps.perm ? kLifp64 : kKronGemm;
  } else {
    if ((size_t)D * M * sizeof(double) > 32 * 1024) return fail(QT_ERR_UNSUPPORTED, "POVM has too many rows for the process kernel");
    if (D == 16 && ps.perm && !h->proc_dense) *path = kLifp16;
    else if (D == 16 && B >= 256 && gemm_lds <= 152 * 1024) *path = kDenseGemm;
    else *path = kFused;  // k_lifp_batch: the one kernel that projects by itself
  }
  return 0;
}

// The writers that form hs_dst(Choi, centre) on the matrix they hold (k_cptp_wave16: n = 2 where a projection launch
// follows the inversion; k_lifp16: n = 2 without the projection; k_lifp_batch<4>: n = 1); every other one -- all of
// n = 3, k_lifp_gemm without the projection, k_lifp_batch<16> -- stores the matrices and k_hs_dist reads them.
bool lifp_dist_in_kernel(const qt_handle_t* h, LifpPath path, int cptp) {
  return h->D == 4 || (h->D == 16 && (path == kLifp16 || (cptp && path != kFused)));
}

// Linear inversion (+ projection) of B processes on device arrays along `path`; `dist` non-null (only where
// lifp_dist_in_kernel): the distances from the same launches, process b to centre (g0 + b) % G of the table `centre`
// (qt::centre_of), and `dchoi` may then be null.
int lifp_launch(qt_handle_t* h, LifpPath path, const int64_t* dc, int B, int cptp, const double* centre, int G, int g0,
                double* dchoi, double* dist, int32_t* dit, int32_t* dst) {
  const int D = h->D, M = h->M;
  const ProcessState& ps = h->proc;
  // R doubles of frequencies per process, Rp with the pitch k_lifp_freq pads to (at n = 3 R is a multiple of 64 already
  // and the factored GEMM reads the rows unpadded).
  const int R = D * M, Rp = ps.factored ? R : (R + 63) / 64 * 64;
  const size_t dyn = (size_t)D * M * sizeof(double);
  const size_t gemm_lds = ((size_t)Rp * 16 + 4 * 256) * sizeof(double);
  const size_t gemm_lds2 = ((size_t)Rp * 32 + 4 * 512) * sizeof(double);  // two column tiles per workgroup
  // The linear inversion into `raw`: the caller's array, or -- when a projection follows -- a workspace; the projection
  // then reports iters, status and the distance, and the inversion gets none of them.
  const bool then_project = cptp && path != kFused;
  double *raw = dchoi, *rdist = dist;
  int32_t *rst = dst, *rit = dit;
  if (then_project) {
    HIPCHK(h->ws_f.ensure((size_t)B * D * D * 2 * sizeof(double)));
    raw = h->ws_f.as<double>();
    rst = rit = nullptr;
    rdist = nullptr;
  }
  double* F = nullptr;  // [B][Rp] frequencies (+ the zeros k_lifp_freq appends) of the two GEMM paths
  if (path == kKronGemm || path == kDenseGemm) {
    HIPCHK(h->ws_x.ensure(((size_t)B * Rp + 192) * sizeof(double)));
    F = h->ws_x.as<double>();
    if (int r = launch(h, qt::k_lifp_freq, dim3((B * D + 15) / 16), dim3(256), 0, dc, B * D, M, D, Rp, F)) return r;
  }
  switch (path) {
    case kLifp64:  // M % 4 == 0: both products of a process in one kernel on the matrix cores
      if (int r = launch(h, qt::k_lifp64, dim3(4 * B), dim3(256), 0, dc, B, M, ps.vp_perm.as<double>(), ps.vs_pinv.as<double>(),
                         raw, rst, rit))
        return r;
      break;
    case kKronGemm: {
      HIPCHK(h->ws_g.ensure((size_t)B * D * D * 2 * sizeof(double)));
      double* T = h->ws_g.as<double>();
      // T[(b, s)][beta] = sum_m F[(b, s)][m] V_P^+[beta][m]: real x complex = a real GEMM with 2 D interleaved columns
      for (int b0 = 0; b0 < B; b0 += 8192) {  // (grid.y <= 65535 row tiles)
        const int nb = B - b0 < 8192 ? B - b0 : 8192;
        if (int r = launch(h, qt::k_gemm<0>, dim3(2 * D / 16, (nb * D + 15) / 16), dim3(64), 0, nb * D, 2 * D, M, F + (size_t)b0 * R,
                           M, 0, ps.vp_pinvT.as<double>(), 2 * D, 0, T + (size_t)b0 * D * D * 2, 2 * D))
          return r;
      }
      if (int r = launch(h, qt::k_lifp_kron_finish, dim3(B), dim3(256), 0, T, ps.vs_pinv.as<double>(), B, raw, rst, rit)) return r;
      break;
    }
    case kLifp16: {  // n = 2 through the Kronecker factors of the left inverse: one wavefront per process (qt_process.h).
      // At most 768 workgroups, three resident per CU (166 VGPRs): the wavefronts stride over the batch with the next
      // process's counts in flight, and a workgroup stages V_P^+ once for all its processes.  The distance takes a
      // 16 x 17 complex transpose scratch per wavefront behind V_P^+
      const size_t lds = (size_t)M * 32 * sizeof(double) + (rdist ? 4 * 16 * 17 * 2 * sizeof(double) : 0);
      if (int r = launch(h, M == 36 ? qt::k_lifp16<9> : qt::k_lifp16<0>, dim3(std::min((B + 3) / 4, 768)), dim3(256), lds, dc, B, M,
                         ps.vp_perm.as<double>(), ps.vs_pinv.as<double>(), raw, rst, rit, centre, G, g0, rdist))
        return r;
      break;
    }
    case kDenseGemm: {  // many processes: frequencies, then one FP64 MFMA GEMM over the batch
      constexpr int NE = 256;
      // 4 groups of 16 processes per workgroup pass (x 2 halves of K).  A workgroup keeps its operand slice for up
      // to 4 passes once there are enough blocks to fill the chip anyway (measured: B = 1024 best with 1-2 passes,
      // 26 M/s; B = 8192 with 4, 38 M/s against 35 M/s with 1)
      const int nblocks = (B + 63) / 64;
      const int passes = nblocks >= 64 ? 4 : (nblocks >= 32 ? 2 : 1);
      const int row_blocks = (nblocks + passes - 1) / passes;
      const bool two = gemm_lds2 <= kLdsLimit;  // two column tiles per workgroup: half the re-reads of F (R <= 576)
      auto kern = two ? qt::k_lifp_gemm<16, 2> : qt::k_lifp_gemm<16, 1>;
#ifdef QT_PHASE_TIMING
      switch (two ? g_host_diag : 0) {  // profile build: a compile-time variant of the two-tile kernel (qt_debug_set_diag)
        case 0: break;
        case 1: kern = qt::k_lifp_gemm<16, 2, 1>; break;
        case 2: kern = qt::k_lifp_gemm<16, 2, 2>; break;
        case 3: kern = qt::k_lifp_gemm<16, 2, 3>; break;
        case 4: kern = qt::k_lifp_gemm<16, 2, 4>; break;
        case 7: kern = qt::k_lifp_gemm<16, 2, 7>; break;
        case 8: kern = qt::k_lifp_gemm<16, 2, 8>; break;
        case 15: kern = qt::k_lifp_gemm<16, 2, 15>; break;
        default: return fail(QT_ERR_ARG, "no such diagnostic variant");
      }
#endif
      if (int r = launch(h, kern, dim3(2 * NE / (two ? 32 : 16), row_blocks), dim3(512), two ? gemm_lds2 : gemm_lds, F, B, R, Rp,
                         ps.pinvR.as<double>(), raw, rst, rit))
        return r;
      break;
    }
    case kFused:
      if (int r = launch(h, D == 4 ? qt::k_lifp_batch<4> : qt::k_lifp_batch<16>, dim3(B),
                         dim3(D == 4 ? qt::ProcWG<4>::NT : qt::ProcWG<16>::NT), dyn, dc, B, M, ps.pinvT.as<double>(), cptp, dchoi,
                         dit, dst, centre, G, g0, dist))
        return r;
      break;
  }
  // The projection, where the path left it to do.
  if (then_project)
    if (int r = project(h, raw, B, 0, 1000, 1e-12, dchoi, dit, dst, centre, G, g0, dist)) return r;
  return 0;
}

// The three entry points.  `with_dist` false: qt_lifp_batch.  Otherwise `centre` holds G matrices, process b is measured
// against centre b % G (qt_lifp_dist_batch: G = 1), and the batch runs in slices (QT_OPT_LIFP_DIST_SLICE) that bound
// every workspace whose size follows the batch: the raw inversion a projection reads, and -- where k_hs_dist forms the
// distance and the caller wants no matrices -- the matrices themselves.
int lifp_batch_impl(qt_handle_t* h, bool with_dist, const int64_t* counts, int B, int cptp, const double* centre, int G,
                    double* choi, double* dist, int32_t* iters, int32_t* status, int flags, const char* fn) {
  QT_ENTER(h);
  Call c(h, flags, fn);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (B < 0 || G < 1 || (B > 0 && (!counts || (with_dist ? !centre || !dist : !choi))))
    return fail(QT_ERR_ARG, "bad %s arguments", fn + 3);
  if (B == 0) return 0;
  if (!with_dist) dist = nullptr;
  const int D = h->D, M = h->M;
  const size_t ne2 = (size_t)D * D * 2;
  const int64_t* dc;
  const double* dcen;
  double *dchoi, *ddist;
  int32_t *dit, *dst;
  if (int r = c.in(counts, (size_t)B * D * M, &dc)) return r;
  if (int r = c.in(centre, dist ? (size_t)G * ne2 : 0, &dcen)) return r;
  if (int r = c.out(choi, (size_t)B * ne2, &dchoi)) return r;
  if (int r = c.out(dist, (size_t)B, &ddist)) return r;
  if (int r = c.out(iters, (size_t)B, &dit)) return r;
  if (int r = c.out(status, (size_t)B, &dst)) return r;
  LifpPath path;
  if (int r = lifp_path(h, B, &path)) return r;
  if (!dist) {
    if (int r = lifp_launch(h, path, dc, B, cptp, nullptr, 1, 0, dchoi, nullptr, dit, dst)) return r;
    return c.done(status, B);
  }
  constexpr size_t kSliceBytes = (size_t)128 << 20;  // of Choi matrices: 2048 processes at n = 3, 32 768 at n = 2
  const int cap = (int)(kSliceBytes / (ne2 * sizeof(double)));
  const int slice = h->lifp_dist_slice > 0 && h->lifp_dist_slice < cap ? h->lifp_dist_slice : cap;
  const bool in_kernel = lifp_dist_in_kernel(h, path, cptp);
  for (int b0 = 0; b0 < B; b0 += slice) {
    const int nb = B - b0 < slice ? B - b0 : slice;
    const int g0 = b0 % G;  // the group of the slice's first process
    double* m = dchoi ? dchoi + (size_t)b0 * ne2 : nullptr;
    if (!in_kernel && !m) {
      HIPCHK(h->lifp_dist_ws.ensure((size_t)nb * ne2 * sizeof(double)));
      m = h->lifp_dist_ws.as<double>();
    }
    if (int r = lifp_launch(h, path, dc + (size_t)b0 * D * M, nb, cptp, dcen, G, g0, m, in_kernel ? ddist + b0 : nullptr,
                            dit ? dit + b0 : nullptr, dst ? dst + b0 : nullptr))
      return r;
    if (!in_kernel)
      if (int r = launch(h, qt::k_hs_dist, dim3(nb), dim3(64), 0, D, (const double*)m, dcen, G, g0, nb, ddist + b0)) return r;
  }
  return c.done(status, B);
}

// dist[b] = metric(rho[b], centre (g0 + b) % G) for 2^NQ x 2^NQ matrices, NQ <= 3, all pointers on the device
// (k_metric_dist; the infidelity's roots of the centres by k_psd_sqrt into metric_ws, once per call)
template <int NQ>
int metric_small(qt_handle_t* h, int metric, const double* dr, int B, const double* dcn, int G, int g0, double* dd) {
  using S = qt::Small<NQ>;
  const dim3 grid((B + S::TPB - 1) / S::TPB), block(S::NT);
  if (metric == QT_METRIC_TRACE)
    return launch(h, qt::k_metric_dist<NQ, qt::kMetricTrace>, grid, block, 0, dr, B, dcn, G, g0, h->jtol2, dd);
  HIPCHK(h->metric_ws.ensure((size_t)G * S::D * 2 * sizeof(double)));
  double* roots = h->metric_ws.as<double>();
  if (int r = launch(h, qt::k_psd_sqrt<NQ>, dim3((G + S::TPB - 1) / S::TPB), block, 0, dcn, G, h->jtol2, roots)) return r;
  return launch(h, qt::k_metric_dist<NQ, qt::kMetricInfidelity>, grid, block, 0, dr, B, static_cast<const double*>(roots), G,
                g0, h->jtol2, dd);
}

// The same for DIM = 16, 32: one workgroup of DIM^2 threads per trial and per centre (k_metric_dist_dim, k_psd_sqrt_dim)
template <int DIM>
int metric_dim(qt_handle_t* h, int metric, const double* dr, int B, const double* dcn, int G, int g0, double* dd) {
  const dim3 block(DIM * DIM);
  if (metric == QT_METRIC_TRACE)
    return launch(h, qt::k_metric_dist_dim<DIM, qt::kMetricTrace>, dim3(B), block, 0, dr, B, dcn, G, g0, h->jtol2, dd);
  HIPCHK(h->metric_ws.ensure((size_t)G * DIM * DIM * 2 * sizeof(double)));
  double* roots = h->metric_ws.as<double>();
  if (int r = launch(h, qt::k_psd_sqrt_dim<DIM>, dim3(G), block, 0, dcn, G, h->jtol2, roots)) return r;
  return launch(h, qt::k_metric_dist_dim<DIM, qt::kMetricInfidelity>, dim3(B), block, 0, dr, B,
                static_cast<const double*>(roots), G, g0, h->jtol2, dd);
}

// The same for dim 64: one workgroup of 1024 threads per trial and per centre, four elements per thread, dynamic LDS
// (k_metric_dist_dim64, k_psd_sqrt_dim64)
int metric_dim64(qt_handle_t* h, int metric, const double* dr, int B, const double* dcn, int G, int g0, double* dd) {
  using W = qt::MetricDim64;
  const dim3 block(W::NT);
  if (metric == QT_METRIC_TRACE)
    return launch(h, qt::k_metric_dist_dim64<qt::kMetricTrace>, dim3(B), block, W::kLdsBytes, dr, B, dcn, G, g0, h->jtol2, dd);
  HIPCHK(h->metric_ws.ensure((size_t)G * W::NE * 2 * sizeof(double)));
  double* roots = h->metric_ws.as<double>();
  if (int r = launch(h, qt::k_psd_sqrt_dim64, dim3(G), block, W::kLdsBytes, dcn, G, h->jtol2, roots)) return r;
  return launch(h, qt::k_metric_dist_dim64<qt::kMetricInfidelity>, dim3(B), block, W::kLdsBytes, dr, B,
                static_cast<const double*>(roots), G, g0, h->jtol2, dd);
}

// The device arrays of a fused chain call, as staged by mhmc_hits_call
struct MhmcHitsArgs {
  const int64_t* counts;
  const double *centres, *init, *thresholds;
  int64_t *hits, *accepted;
  double* dist;
  uint32_t burn_steps, n_points, thinning;
};

// Elements per chain of its counts, of its centre and of its starting point
struct MhmcHitsElems {
  size_t counts, centre, init;
};

// The six entries of the fused chains (`hs`: the metric is not read): the same checks and staging.  `refuse(elems)` makes
// the entry's own refusals, in its order, and states the sizes of a chain; `launch_chains(args)` enqueues its kernels.
template <class Refuse, class Launch>
int mhmc_hits_call(qt_handle_t* h, const char* fn, bool hs, int metric, const int64_t* counts, int C, const double* centres,
                   const double* init, const double* thresholds, int burn_steps, int n_points, int thinning, int64_t* hits,
                   int64_t* accepted, double* dist, int flags, Refuse refuse, Launch launch_chains) {
  QT_ENTER(h);
  Call c(h, flags, fn);
  MhmcHitsElems n{};
  if (int r = refuse(n)) return r;
  if (!hs && metric != QT_METRIC_TRACE && metric != QT_METRIC_INFIDELITY)
    return fail(QT_ERR_ARG, "%s: unknown metric %d", fn, metric);
  if (C < 0 || burn_steps < 0 || n_points < 0 || thinning < 1 ||
      (C > 0 && (!counts || !centres || !init || !thresholds || !hits || !accepted)))
    return fail(QT_ERR_ARG, "bad %s arguments", fn + 3);
  if ((uint64_t)burn_steps + (uint64_t)n_points * (uint64_t)thinning >= 0xffffffffull)
    return fail(QT_ERR_ARG, "%s: burn_steps + n_points * thinning must be below 2^32 - 1", fn);
  if (C == 0) return 0;
  MhmcHitsArgs a{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (uint32_t)burn_steps, (uint32_t)n_points,
                 (uint32_t)thinning};
  if (int r = c.in(counts, (size_t)C * n.counts, &a.counts)) return r;
  if (int r = c.in(centres, (size_t)C * n.centre, &a.centres)) return r;
  if (int r = c.in(init, (size_t)C * n.init, &a.init)) return r;
  if (int r = c.in(thresholds, (size_t)C, &a.thresholds)) return r;
  if (int r = c.out(hits, (size_t)C, &a.hits)) return r;
  if (int r = c.out(accepted, (size_t)C, &a.accepted)) return r;
  if (int r = c.out(dist, (size_t)C * n_points, &a.dist)) return r;
  if (int r = launch_chains(a)) return r;
  return c.done();
}

}  // namespace

// qt_lp_pieces.hip: the kernel of qt_lp_pieces is compiled on its own, so that the LP kernels here do not depend on it
namespace qt {
void lp_pieces_launch(int kernel, hipStream_t stream, const double* A, int M, int N, const double* w, const double* vm,
                      const double* vn, int p1, int mode, double* normal, double* factor, double* u, double* ax,
                      double* solved, int32_t* ok, double* ws);
}

extern "C" {

int qt_version(void) { return 100; }

const char* qt_last_error(void) { return g_err.c_str(); }

int qt_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(QT_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  return n;
}

qt_handle_t* qt_create(int device, int n_qubits) {
  if (n_qubits < 1 || n_qubits > 5) {
    fail(QT_ERR_ARG, "n_qubits must be in 1..5 (got %d)", n_qubits);
    return nullptr;
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    fail(QT_ERR_HIP, "no usable HIP device (%s); this library has no CPU path", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= n) {
    fail(QT_ERR_ARG, "device %d out of range (have %d)", device, n);
    return nullptr;
  }
  DeviceScope scope(device);
  if (scope.err != hipSuccess) {
    fail(QT_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(scope.err));
    return nullptr;
  }
  qt_handle_t* h = new qt_handle();
  h->device = device;
  h->nq = n_qubits;
  h->d = 1 << n_qubits;
  h->D = h->d * h->d;
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreate(&h->ev0)) != hipSuccess || (e = hipEventCreate(&h->ev1)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->ev_sync, hipEventDisableTiming)) != hipSuccess) {
    fail(QT_ERR_HIP, "stream/event creation: %s", hipGetErrorString(e));
    delete h;
    return nullptr;
  }
  h->own_stream = true;
  if (const char* env = getenv("QTOMO_SKIP_SHOTS_CHECK")) h->check_shots = !(env[0] == '1');
  return h;
}

void qt_destroy(qt_handle_t* h) {
  if (!h) return;
  DeviceScope scope(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->povm.release();
  for (DevBuf* b : {&h->info, &h->kron_dig, &h->aug, &h->proc_ws, &h->lifp_dist_ws, &h->born_ws,
                    &h->gram, &h->moment_freq, &h->moment_part, &h->moment_qpart, &h->poly_ws, &h->metric_ws, &h->mhmc_parked, &h->ws_x, &h->ws_g, &h->ws_f, &h->ws_act, &h->hess, &h->sort_alt, &h->sort_tmp,
                    &h->sc_ok, &h->sc_fail, &h->sc_pos, &h->sc_tmp, &h->sc_in, &h->sc_out, &h->sc_iters, &h->sc_choi,
                    &h->lp_ws, &h->lp_large_ws, &h->lp_xl_ws})
    b->release();
  for (DevBuf& b : h->stage) b.release();
  h->proc.release();
  if (h->mail) (void)hipHostFree(h->mail);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->ev_sync) (void)hipEventDestroy(h->ev_sync);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int qt_sync(qt_handle_t* h) {
  QT_ENTER(h);
  return wait_stream(h);
}

int qt_set_stream(qt_handle_t* h, void* hip_stream) {
  QT_ENTER(h);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->own_stream && h->stream) HIPCHK(hipStreamDestroy(h->stream));
  if (hip_stream) {
    h->stream = hip_stream == QT_STREAM_LEGACY ? hipStreamLegacy : static_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
  } else {
    HIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  return 0;
}

int qt_set_option(qt_handle_t* h, int option, double value) {
  QT_ENTER(h);
  switch (option) {
    case QT_OPT_SHOTS_CHECK: h->check_shots = value != 0.0; return 0;
    case QT_OPT_MLE_FUSED_MAX_WAVES:
      if (!(value >= 0.0 && value <= 1048576.0)) return fail(QT_ERR_ARG, "QT_OPT_MLE_FUSED_MAX_WAVES out of range");
      h->fused_max_waves = (int)value;
      return 0;
    case QT_OPT_PAIRED_STAGES: h->paired_stages = value != 0.0; return 0;
    case QT_OPT_MLE_SPECIALISE: h->mle_specialise = value != 0.0; return 0;
    case QT_OPT_MLE_HELPER_WAVE: h->mle_helper_wave = value != 0.0; return 0;
    case QT_OPT_LIFP_DIST_SLICE:
      if (!(value >= 0.0 && value <= 16777216.0)) return fail(QT_ERR_ARG, "QT_OPT_LIFP_DIST_SLICE out of range");
      h->lifp_dist_slice = (int)value;
      return 0;
    case QT_OPT_MHMC_PROCESS_SLICE:
      if (!(value >= 0.0 && value <= 16777216.0)) return fail(QT_ERR_ARG, "QT_OPT_MHMC_PROCESS_SLICE out of range");
      h->mhmc_process_slice = (int)value;
      return 0;
    default: return fail(QT_ERR_ARG, "unknown option %d", option);
  }
}

int qt_get_paired_tables(qt_handle_t* h) {
  QT_ENTER(h);
  return h->povm.registered && h->povm.prod.enabled ? h->povm.paired_tables : 0;
}

int qt_get_mle_specialised(qt_handle_t* h) {
  QT_ENTER(h);
  return h->last_mle_spec ? 1 : 0;
}

int qt_get_mle_helper_wave(qt_handle_t* h) {
  QT_ENTER(h);
  return h->last_mle_helper ? 1 : 0;
}

int qt_timer_begin(qt_handle_t* h) {
  QT_ENTER(h);
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  return 0;
}

// the end event only (asynchronous): a caller that synchronises anyway reads the interval afterwards
int qt_timer_stop(qt_handle_t* h) {
  QT_ENTER(h);
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  return 0;
}

int qt_timer_elapsed(qt_handle_t* h, double* elapsed_ms) {
  QT_ENTER(h);
  if (!elapsed_ms) return fail(QT_ERR_ARG, "null elapsed_ms");
  if (int r = wait_event_spin(h->ev1)) return r;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *elapsed_ms = ms;
  return 0;
}

int qt_timer_end(qt_handle_t* h, double* elapsed_ms) {
  if (int r = qt_timer_stop(h)) return r;
  return qt_timer_elapsed(h, elapsed_ms);
}

int qt_pauli_basis(qt_handle_t* h, double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!out) return fail(QT_ERR_ARG, "null out");
  const size_t n = (size_t)h->D * h->D * 2;
  double* dout;
  if (int r = c.out(out, n, &dout)) return r;
  hipLaunchKernelGGL(qt::k_pauli_basis, dim3(grid_for(n / 2)), dim3(256), 0, h->stream, h->nq, dout);
  return c.done();
}

int qt_povm_kron(qt_handle_t* h, const double* povm1, int S1, int K1, double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!povm1 || !out || S1 < 1 || K1 < 1) return fail(QT_ERR_ARG, "bad povm_kron arguments");
  size_t S = 1, K = 1;
  for (int q = 0; q < h->nq; ++q) {
    S *= S1;
    K *= K1;
  }
  const size_t n = S * K * h->D;
  const double* din;
  double* dout;
  if (int r = c.in(povm1, (size_t)S1 * K1 * 4, &din)) return r;
  if (int r = c.out(out, n, &dout)) return r;
  if (int r = launch_povm_kron(h, din, S1, K1, dout)) return r;
  return c.done();
}

int qt_set_povm(qt_handle_t* h, const double* A, int S, int K, const double* Ns, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!A || !Ns || S < 1 || K < 1) return fail(QT_ERR_ARG, "bad set_povm arguments");
  if (int r = begin_povm(h, S, K)) return r;
  PovmState& pm = h->povm;
  HIPCHK(pm.A.ensure((size_t)S * K * h->D * sizeof(double)));
  if (int r = c.copy_in(pm.A.as<double>(), A, (size_t)S * K * h->D)) return r;
  if (int r = c.copy_in(pm.Ns.as<double>(), Ns, (size_t)S)) return r;
  pm.a_loaded = true;
  {
    std::vector<double> ns;
    if (int r = c.read(ns, Ns, (size_t)S)) return r;
    for (double v : ns) pm.ns_tot += v;
  }
  if (int r = compute_dense_pinv(h)) return r;  // a plain tensor: the dense operands ARE the POVM
  pm.registered = true;
  return 0;
}

int qt_set_povm_product(qt_handle_t* h, const double* povm1, int S1, int K1, const double* Ns, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!povm1 || !Ns || S1 < 1 || K1 < 1) return fail(QT_ERR_ARG, "bad set_povm_product arguments");
  const int n = h->nq;
  auto refused = [](qt::TablesStatus st, const qt::ProductShape& sh) {
    if (st == qt::TABLES_ROWS) return fail(QT_ERR_UNSUPPORTED, "product POVM with %lld rows is too large", sh.M);
    return fail(QT_ERR_UNSUPPORTED, "one-qubit table with %lld rows (> 255)", sh.R1);
  };
  qt::ProductTables tb;
  if (qt::TablesStatus st = qt::product_shape(n, S1, K1, &tb.shape)) return refused(st, tb.shape);
  const int R1 = (int)tb.shape.R1;
  if (int r = begin_povm(h, (int)tb.shape.S, (int)tb.shape.K)) return r;
  PovmState& pm = h->povm;
  // host copies of the small inputs (table and shots), and the index tables from them
  std::vector<double> t1, ns;
  if (int r = c.read(t1, povm1, (size_t)R1 * 4)) return r;
  if (int r = c.read(ns, Ns, (size_t)tb.shape.S)) return r;
  if (qt::TablesStatus st = qt::build_product_tables(n, S1, K1, ns.data(), t1.data(), &tb)) return refused(st, tb.shape);
  if (int r = upload(h, pm.T, t1)) return r;
  if (int r = upload(h, pm.Ns, ns)) return r;
  pm.ns_tot = tb.tot;
  pm.ns_max = tb.ns_max;
  pm.S1 = S1;
  pm.K1 = K1;
  // The dense operands (a2 tensor + transposes; Born GEMM, dense fallbacks, process set-up) are cheap at n <= 3 and
  // built now; at n = 4, 5 (6 x 64 MB at n = 5) the factorised estimators never read them: on demand only.
  // The dense left inverse is needed by 'lin' when the shots differ between settings (n <= 3).
  if (n <= 3) {
    if (int r = tb.uniform ? ensure_dense(h) : compute_dense_pinv(h)) return r;
  }
  // pinv of the one-qubit table, on the device: inv(T^T T) T^T  ([4][R1]) and its transpose
  HIPCHK(pm.P1.ensure((size_t)4 * R1 * sizeof(double)));
  HIPCHK(pm.P1T.ensure((size_t)4 * R1 * sizeof(double)));
  if (int r = enqueue_left_inverse<1>(h, pm.T.as<double>(), R1, 4, pm.P1.as<double>())) return r;
  if (int r = launch_transpose<1>(h, pm.P1.as<double>(), 4, R1, pm.P1T.as<double>())) return r;
  if (int r = upload(h, pm.rinv, tb.rinv)) return r;
  if (int r = upload(h, pm.rmap, tb.rmap)) return r;
  if (int r = upload(h, pm.wrow, tb.wrow)) return r;
  if (int r = upload(h, pm.fwd, tb.fwd)) return r;
  if (int r = upload(h, pm.bwd, tb.bwd)) return r;
  if (int r = upload(h, pm.last, tb.last)) return r;
  // The pivot report and, for the shape that has paired stages, pinv(T)^T: it is classified on the values the kernels
  // read, i.e. on the device's result.
  int info = 0;
  double p1t[24] = {};
  HIPCHK(hipMemcpyAsync(&info, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (tb.try_paired) HIPCHK(hipMemcpyAsync(p1t, pm.P1T.p, sizeof(p1t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  if (info != 0) return fail(QT_ERR_SINGULAR, "the one-qubit table is not informationally complete");
  qt::ProductView pv{};
  pv.T = pm.T.as<double>();
  pv.P1T = pm.P1T.as<double>();
  pv.wrowR = pm.wrow.as<double>();
  pv.rmap = pm.rmap.as<int>();
  pv.rinv = pm.rinv.as<int>();
  pv.fwd = pm.fwd.as<int>();
  pv.bwd = pm.bwd.as<int>();
  pv.last = pm.last.as<int>();
  pv.R1 = R1;
  pv.uniform = tb.uniform ? 1 : 0;
  pv.wuni = tb.wuni;
  pv.enabled = 1;
  if (tb.try_paired) {
    const qt::PairedTables pt = qt::classify_paired(tb, p1t);
    memcpy(pv.cT, pt.cT, sizeof pv.cT);
    memcpy(pv.cP, pt.cP, sizeof pv.cP);
    pm.paired_tables = (tb.pairedT ? 1 : 0) | (pt.pairedP ? 2 : 0);
    if (!pt.image.empty()) {
      if (int r = upload(h, pm.image, pt.image)) return r;
      HIPCHK(hipStreamSynchronize(h->stream));  // `pt` goes out of scope
      pm.image_ready = true;
    }
  }
  pm.prod = pv;
  pm.registered = true;
  return 0;
}

int qt_get_left_inverse(qt_handle_t* h, double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (!out) return fail(QT_ERR_ARG, "null out");
  if (!h->povm.pinv_ready)
    if (int r = compute_dense_pinv(h)) return r;
  if (int r = c.copy_out(out, h->povm.Pinv.as<double>(), (size_t)h->D * h->M)) return r;
  return c.done();
}

int qt_born_probs(qt_handle_t* h, const double* bloch, int B, double* p, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (B < 0 || (B > 0 && (!bloch || !p))) return fail(QT_ERR_ARG, "bad born_probs arguments");
  if (B == 0) return 0;
  const double* din;
  double* dout;
  if (int r = c.in(bloch, (size_t)B * h->D, &din)) return r;
  if (int r = c.out(p, (size_t)B * h->M, &dout)) return r;
  if (int r = born_launch(h, din, B, dout)) return r;
  return c.done();
}

int qt_bloch_from_mat(qt_handle_t* h, const double* mat, int B, double* bloch, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || (B > 0 && (!mat || !bloch))) return fail(QT_ERR_ARG, "bad bloch_from_mat arguments");
  if (B == 0) return 0;
  const double* din;
  double* dout;
  const size_t n = (size_t)B * h->D;
  if (int r = c.in(mat, n * 2, &din)) return r;
  if (int r = c.out(bloch, n, &dout)) return r;
  hipLaunchKernelGGL(qt::k_bloch_from_mat, dim3(grid_for(n)), dim3(256), 0, h->stream, h->nq, din, B, dout);
  return c.done();
}

int qt_mat_from_bloch(qt_handle_t* h, const double* bloch, int B, double* mat, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || (B > 0 && (!mat || !bloch))) return fail(QT_ERR_ARG, "bad mat_from_bloch arguments");
  if (B == 0) return 0;
  const double* din;
  double* dout;
  const size_t n = (size_t)B * h->D;
  if (int r = c.in(bloch, n, &din)) return r;
  if (int r = c.out(mat, n * 2, &dout)) return r;
  hipLaunchKernelGGL(qt::k_mat_from_bloch, dim3(grid_for(n)), dim3(256), 0, h->stream, h->nq, din, B, dout);
  return c.done();
}

int qt_lin_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, double* rho, double* bloch_out,
                 int32_t* status, int flags) {
  if (B > 0 && !rho) return fail(QT_ERR_ARG, "bad lin_batch arguments");
  return lin_batch_impl(h, counts, B, physical, nullptr, 1, rho, nullptr, bloch_out, status, flags);
}

int qt_lin_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, const double* centre, double* rho,
                      double* dist, int32_t* status, int flags) {
  if (B > 0 && (!dist || !centre)) return fail(QT_ERR_ARG, "bad lin_dist_batch arguments");
  return lin_batch_impl(h, counts, B, physical, centre, 1, rho, dist, nullptr, status, flags);
}

int qt_lin_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int physical, const double* centres, int G,
                            double* rho, double* dist, int32_t* status, int flags) {
  if (G < 1 || (B > 0 && (!dist || !centres))) return fail(QT_ERR_ARG, "bad lin_dist_group_batch arguments");
  return lin_batch_impl(h, counts, B, physical, centres, G, rho, dist, nullptr, status, flags);
}

int qt_chol_param(qt_handle_t* h, const double* rho, int B, double* x, int32_t* status, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || (B > 0 && (!rho || !x))) return fail(QT_ERR_ARG, "bad chol_param arguments");
  if (B == 0) return 0;
  const double* din;
  double* dx;
  int32_t* dst;
  const size_t nel = (size_t)B * h->D;
  if (int r = c.in(rho, nel * 2, &din)) return r;
  if (int r = c.out(x, nel, &dx)) return r;
  if (int r = c.out(status, (size_t)B, &dst)) return r;
  if (int r = by_nq(h, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const Plan p = chol_plan<NQ>(h, B);
        if constexpr (NQ <= 3) return launch(h, qt::k_chol_param<NQ>, p, p.pv, din, B, dx, dst);
        else return launch(h, qt::k_chol_param_large<NQ>, p, p.pv, din, B, dx, dst);
      }))
    return r;
  return c.done(status, B);
}

int qt_chol_unparam(qt_handle_t* h, const double* x, int B, double* LLh, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || (B > 0 && (!x || !LLh))) return fail(QT_ERR_ARG, "bad chol_unparam arguments");
  if (B == 0) return 0;
  const double* din;
  double* dout;
  const size_t nel = (size_t)B * h->D;
  if (int r = c.in(x, nel, &din)) return r;
  if (int r = c.out(LLh, nel * 2, &dout)) return r;
  if (int r = by_nq(h, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const Plan p = chol_plan<NQ>(h, B);
        if constexpr (NQ <= 3) return launch(h, qt::k_chol_unparam<NQ>, p, p.pv, din, B, dout);
        else return launch(h, qt::k_chol_unparam_large<NQ>, p, p.pv, din, B, dout);
      }))
    return r;
  return c.done();
}

int qt_nll_batch(qt_handle_t* h, const double* x, const int64_t* counts, int B, double* f, double* grad, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (B < 0 || (B > 0 && (!x || !counts || !f))) return fail(QT_ERR_ARG, "bad nll_batch arguments");
  if (B == 0) return 0;
  const double* dx;
  const int64_t* dc;
  double *df, *dg;
  const size_t nel = (size_t)B * h->D;
  if (int r = c.in(x, nel, &dx)) return r;
  if (int r = c.in(counts, (size_t)B * h->M, &dc)) return r;
  if (int r = c.out(f, (size_t)B, &df)) return r;
  if (int r = c.out(grad, nel, &dg)) return r;
  if (int r = by_nq(h, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const Plan p = povm_plan<NQ>(h, B);
        if constexpr (NQ <= 3) return launch(h, qt::k_nll_batch<NQ>, p, p.pv, dx, dc, B, df, dg);
        else return launch(h, qt::k_nll_large<NQ>, p, p.pv, dx, dc, B, df, dg);
      }))
    return r;
  return c.done();
}

int qt_mhmc_state(qt_handle_t* h, const int64_t* counts, int C, const double* x_init, const double* deltas,
                  const double* uniforms, int T, double step, double* chain, int32_t* accepted, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (C < 0 || T < 0 || (C > 0 && T > 0 && (!counts || !x_init || !deltas || !uniforms || !chain || !accepted)))
    return fail(QT_ERR_ARG, "bad mhmc_state arguments");
  if (C == 0 || T == 0) return 0;
  const int64_t* dc;
  const double *dx, *dd, *du;
  double* dch;
  int32_t* dacc;
  const size_t nel = (size_t)C * T * h->D;
  if (int r = c.in(counts, (size_t)C * h->M, &dc)) return r;
  if (int r = c.in(x_init, (size_t)C * h->D, &dx)) return r;
  if (int r = c.in(deltas, nel, &dd)) return r;
  if (int r = c.in(uniforms, (size_t)C * T, &du)) return r;
  if (int r = c.out(chain, nel, &dch)) return r;
  if (int r = c.out(accepted, (size_t)C * T, &dacc)) return r;
  if (int r = by_nq(h, [&](auto nq) {
        constexpr int NQ = decltype(nq)::value;
        const Plan p = povm_plan<NQ>(h, C);
        if constexpr (NQ <= 3) return launch(h, qt::k_mhmc_state<NQ>, p, p.pv, dc, C, dx, dd, du, T, step, dch, dacc);
        else return launch(h, qt::k_mhmc_state_large<NQ>, p, p.pv, dc, C, dx, dd, du, T, step, dch, dacc);
      }))
    return r;
  return c.done();
}

// The entries of the state chain whose numbers are drawn on the device (qt_sampler::mhmc_draw) that serve n <= 3 only
static int mhmc_device_nq(const qt_handle_t* h, const char* fn) {
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "%s supports n_qubits 1..3 (got %d): the device-drawn chain has no n = 4, 5 kernel", fn, h->nq);
  return 0;
}

// The three entries of the draws, behind their own preconditions: deltas[C][T][len] and uniforms[C][T]
static int mhmc_draws_call(qt_handle_t* h, const char* fn, int len, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step,
                           int T, double* deltas, double* uniforms, int flags) {
  Call c(h, flags, fn);
  if (C < 0 || T < 0 || (C > 0 && T > 0 && (!deltas || !uniforms))) return fail(QT_ERR_ARG, "bad %s arguments", fn + 3);
  if ((uint64_t)first_step + (uint64_t)T >= 0xffffffffull) return fail(QT_ERR_ARG, "%s: steps beyond 2^32 - 2", fn);
  if (C == 0 || T == 0) return 0;
  double *dd, *du;
  const size_t ct = (size_t)C * T;
  if (int r = c.out(deltas, ct * len, &dd)) return r;
  if (int r = c.out(uniforms, ct, &du)) return r;
  if (int r = launch(h, qt_sampler::k_mhmc_draws, dim3(grid_for(ct * (len + 1), 256, 1 << 16)), dim3(256), 0, seed, first_chain,
                     C, first_step, T, len, dd, du))
    return r;
  return c.done();
}

int qt_mhmc_draws(qt_handle_t* h, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T, double* deltas,
                  double* uniforms, int flags) {
  QT_ENTER(h);
  if (int r = mhmc_device_nq(h, "qt_mhmc_draws")) return r;
  return mhmc_draws_call(h, "qt_mhmc_draws", h->D, seed, first_chain, C, first_step, T, deltas, uniforms, flags);
}

// qt_mhmc_state_hits and qt_mhmc_state_metric_hits (mhmc_hits_call), n <= 3: the plan of the estimators, the infidelity's
// roots of the C centres by k_psd_sqrt into metric_ws first, as metric_small has them
static int mhmc_state_hits_small(qt_handle_t* h, const char* fn, bool hs, int metric, const int64_t* counts, int C, const double* centres,
                                 const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                 int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                                 double* dist, int flags) {
  auto refuse = [&](MhmcHitsElems& n) {
    if (int r = mhmc_device_nq(h, fn)) return r;
    n = {(size_t)h->M, (size_t)h->D * 2, (size_t)h->D};
    return need_povm(h);
  };
  auto launch_chains = [&](const MhmcHitsArgs& a) {
    return by_nq(h, [&](auto nq) {
      constexpr int NQ = decltype(nq)::value;
      if constexpr (NQ <= 3) {
        using S = qt::Small<NQ>;
        const Plan p = povm_plan<NQ>(h, C);
        if (hs)
          return launch(h, qt::k_mhmc_state_hits<NQ>, p, p.pv, a.counts, C, a.centres, a.init, a.thresholds, seed, first_chain,
                        a.burn_steps, a.n_points, a.thinning, step, a.hits, a.accepted, a.dist);
        if (metric == QT_METRIC_TRACE)
          return launch(h, qt::k_mhmc_state_metric_hits<NQ, qt::kMetricTrace>, p, p.pv, a.counts, C, a.centres, a.init,
                        a.thresholds, seed, first_chain, a.burn_steps, a.n_points, a.thinning, step, a.hits, a.accepted, a.dist);
        HIPCHK(h->metric_ws.ensure((size_t)C * S::D * 2 * sizeof(double)));
        double* roots = h->metric_ws.as<double>();
        if (int r = launch(h, qt::k_psd_sqrt<NQ>, dim3((C + S::TPB - 1) / S::TPB), dim3(S::NT), 0, a.centres, C, h->jtol2, roots))
          return r;
        return launch(h, qt::k_mhmc_state_metric_hits<NQ, qt::kMetricInfidelity>, p, p.pv, a.counts, C,
                      static_cast<const double*>(roots), a.init, a.thresholds, seed, first_chain, a.burn_steps, a.n_points,
                      a.thinning, step, a.hits, a.accepted, a.dist);
      } else {
        return 0;  // (refused above)
      }
    });
  };
  return mhmc_hits_call(h, fn, hs, metric, counts, C, centres, x_init, thresholds, burn_steps, n_points, thinning, hits, accepted,
                        dist, flags, refuse, launch_chains);
}

int qt_mhmc_state_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* x_init,
                       const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                       int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags) {
  return mhmc_state_hits_small(h, "qt_mhmc_state_hits", true, 0, counts, C, centres, x_init, thresholds, seed, first_chain,
                               burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_mhmc_state_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                              const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                              int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                              double* dist, int flags) {
  return mhmc_state_hits_small(h, "qt_mhmc_state_metric_hits", false, metric, counts, C, centres, x_init, thresholds, seed,
                               first_chain, burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_mle_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol, double* rho,
                 int32_t* nit, int32_t* nfev, double* fun, int32_t* status, int flags) {
  if (B > 0 && !rho) return fail(QT_ERR_ARG, "bad mle_batch arguments");
  return mle_batch_impl(h, counts, B, init, max_iter, tol, nullptr, 1, rho, nullptr, nit, nfev, fun, status, flags);
}

int qt_mle_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol,
                      const double* centre, double* rho, double* dist, int32_t* nit, int32_t* nfev, double* fun,
                      int32_t* status, int flags) {
  if (B > 0 && (!dist || !centre)) return fail(QT_ERR_ARG, "bad mle_dist_batch arguments");
  return mle_batch_impl(h, counts, B, init, max_iter, tol, centre, 1, rho, dist, nit, nfev, fun, status, flags);
}

int qt_mle_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int init, int max_iter, double tol,
                            const double* centres, int G, double* rho, double* dist, int32_t* nit, int32_t* nfev,
                            double* fun, int32_t* status, int flags) {
  if (G < 1 || (B > 0 && (!dist || !centres))) return fail(QT_ERR_ARG, "bad mle_dist_group_batch arguments");
  return mle_batch_impl(h, counts, B, init, max_iter, tol, centres, G, rho, dist, nit, nfev, fun, status, flags);
}

// metrics.py:140-144 for a chunk of whole resamples: hits[g] += #{ r : thresholds[g] > dist[r][g] } (k_group_hits)
int qt_group_hits(qt_handle_t* h, const double* dist, int B, int G, const double* thresholds, int64_t* hits, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || G < 1 || B % G != 0 || !thresholds || !hits || (B > 0 && !dist))
    return fail(QT_ERR_ARG, "bad group_hits arguments (B = %d must be a multiple of G = %d)", B, G);
  if (B == 0) return 0;
  const double *dd, *dthr;
  int64_t* dhits;
  if (int r = c.in(dist, (size_t)B, &dd)) return r;
  if (int r = c.in(thresholds, (size_t)G, &dthr)) return r;
  if (int r = c.inout(hits, (size_t)G, &dhits)) return r;
  // column tiles of min(G, 256) x slices of rows: about 2048 workgroups at the most, at least eight passes per slice
  const int R = B / G, cw = G < 256 ? G : 256, rp = 256 / cw, gx = (G + cw - 1) / cw;
  int slices = 2048 / gx;
  if (slices < 1) slices = 1;
  int rows = (R + slices - 1) / slices;
  if (rows < 8 * rp) rows = 8 * rp;
  const int gy = (R + rows - 1) / rows;
  if (int r = launch(h, qt::k_group_hits, dim3(gx, gy), dim3(256), 0, dd, R, G, rows, dthr,
                     reinterpret_cast<unsigned long long*>(dhits)))
    return r;
  return c.done();
}

int qt_hs_dist_batch(qt_handle_t* h, const double* rho, const double* centre, int B, double* dist, int flags) {
  if (!h) return fail(QT_ERR_ARG, "null handle");
  return qt_hs_dist_dim(h, h->d, rho, centre, B, dist, flags);
}

// for dim x dim matrices of any size (the Choi matrices of an n-qubit channel are 4^n x 4^n: 2n-qubit objects)
int qt_hs_dist_dim(qt_handle_t* h, int dim, const double* rho, const double* centre, int B, double* dist, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (dim < 1 || dim > 4096 || B < 0 || (B > 0 && (!rho || !centre || !dist))) return fail(QT_ERR_ARG, "bad hs_dist arguments");
  if (B == 0) return 0;
  const size_t ne = (size_t)dim * dim;
  const double *dr, *dcn;
  double* dd;
  if (int r = c.in(rho, (size_t)B * ne * 2, &dr)) return r;
  if (int r = c.in(centre, ne * 2, &dcn)) return r;
  if (int r = c.out(dist, (size_t)B, &dd)) return r;
  hipLaunchKernelGGL(qt::k_hs_dist, dim3(B), dim3(64), 0, h->stream, dim, dr, dcn, 1, 0, B, dd);
  return c.done();
}

// geometry.py:23-56 for a batch of dim x dim matrices against a table of centres, behind QT_ENTER: dim 2, 4, 8 by
// k_metric_dist, dim 16, 32 by one workgroup per trial (qt_metric_dim.h), dim 64 the same with four elements per thread
// (qt_metric_dim64.h); the infidelity's roots of the centres once per call.  Reads no POVM.  `fn`, the entry, words the
// errors; `max_dim`, 32 or 64, is the largest dim it admits.
static int metric_dist_call(qt_handle_t* h, const char* fn, int max_dim, int metric, int dim, const double* rho, int B,
                            const double* centres, int G, int g0, double* dist, int flags) {
  Call c(h, flags, fn);
  if (metric != QT_METRIC_TRACE && metric != QT_METRIC_INFIDELITY) return fail(QT_ERR_ARG, "%s: unknown metric %d", fn, metric);
  if (dim < 2 || dim > max_dim || (dim & (dim - 1)))
    return fail(QT_ERR_UNSUPPORTED, "%s: dim %d (supported: 2, 4, 8, 16, 32%s)", fn, dim, max_dim == 64 ? ", 64" : "");
  if (B < 0 || G < 1 || g0 < 0 || g0 >= G || (B > 0 && (!rho || !centres || !dist)))
    return fail(QT_ERR_ARG, "bad %s arguments (B = %d, G = %d, g0 = %d)", fn + 3, B, G, g0);
  if (B == 0) return 0;
  const double *dr, *dcn;
  double* dd;
  const size_t ne2 = (size_t)dim * dim * 2;
  if (int r = c.in(rho, (size_t)B * ne2, &dr)) return r;
  if (int r = c.in(centres, (size_t)G * ne2, &dcn)) return r;
  if (int r = c.out(dist, (size_t)B, &dd)) return r;
  int r = 0;
  switch (dim) {
    case 2: r = metric_small<1>(h, metric, dr, B, dcn, G, g0, dd); break;
    case 4: r = metric_small<2>(h, metric, dr, B, dcn, G, g0, dd); break;
    case 8: r = metric_small<3>(h, metric, dr, B, dcn, G, g0, dd); break;
    case 16: r = metric_dim<16>(h, metric, dr, B, dcn, G, g0, dd); break;
    case 32: r = metric_dim<32>(h, metric, dr, B, dcn, G, g0, dd); break;
    default: r = metric_dim64(h, metric, dr, B, dcn, G, g0, dd); break;
  }
  if (r) return r;
  return c.done();
}

// ... of the handle's own size, n <= 3
int qt_metric_dist_group_batch(qt_handle_t* h, int metric, const double* rho, int B, const double* centres, int G, int g0,
                               double* dist, int flags) {
  QT_ENTER(h);
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "qt_metric_dist_group_batch: n_qubits %d (supported: 1, 2, 3)", h->nq);
  return metric_dist_call(h, "qt_metric_dist_group_batch", 32, metric, h->d, rho, B, centres, G, g0, dist, flags);
}

// ... of any supported size on any handle, whatever its n_qubits (dim 2, 4, 8: the same bits as on a handle of that size)
int qt_metric_dist_dim(qt_handle_t* h, int metric, int dim, const double* rho, int B, const double* centres, int G, int g0,
                       double* dist, int flags) {
  QT_ENTER(h);
  return metric_dist_call(h, "qt_metric_dist_dim", 32, metric, dim, rho, B, centres, G, g0, dist, flags);
}

// ... and of dim 64 as well (a three-qubit Choi matrix): below 64 the very code of qt_metric_dist_dim
int qt_metric_dist_mat(qt_handle_t* h, int metric, int dim, const double* rho, int B, const double* centres, int G, int g0,
                       double* dist, int flags) {
  QT_ENTER(h);
  return metric_dist_call(h, "qt_metric_dist_mat", 64, metric, dim, rho, B, centres, G, g0, dist, flags);
}

// ---- a16: interval.py:610-612 ------------------------------------------------------------------------
int qt_sort_f64(qt_handle_t* h, double* x, long long n, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (n < 0 || (n > 0 && !x)) return fail(QT_ERR_ARG, "bad sort arguments");
  if (n > 0x7fffffffLL) return fail(QT_ERR_UNSUPPORTED, "qt_sort_f64 sorts at most 2^31 - 1 values");
  if (n == 0) return 0;
  double* dx;
  if (int r = c.inout(x, (size_t)n, &dx)) return r;
  if (n <= 8192) {  // one workgroup, bitonic network in LDS
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    hipLaunchKernelGGL(qt::k_sort_small, dim3(1), dim3(np2 / 2 < 1024 ? (np2 / 2 < 64 ? 64 : np2 / 2) : 1024), np2 * sizeof(double),
                       h->stream, dx, (int)n, np2);
    return c.done();
  }
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(qt::k_sort_canonical, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, h->stream, dx, n);
  HIPCHK(h->sort_alt.ensure((size_t)n * sizeof(double)));
  hipcub::DoubleBuffer<double> keys(dx, h->sort_alt.as<double>());
  size_t tmp_bytes = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, keys, (int)n, 0, 64, h->stream));
  HIPCHK(h->sort_tmp.ensure(tmp_bytes));
  HIPCHK(hipcub::DeviceRadixSort::SortKeys(h->sort_tmp.p, tmp_bytes, keys, (int)n, 0, 64, h->stream));
  if (keys.Current() != dx)
    HIPCHK(hipMemcpyAsync(dx, keys.Current(), (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return c.done();
}

int qt_sorted_quantiles(qt_handle_t* h, const double* sorted, long long n, const double* conf_levels, int n_levels,
                        double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (n < 1 || n_levels < 0 || !sorted || (n_levels > 0 && (!conf_levels || !out)))
    return fail(QT_ERR_ARG, "bad sorted_quantiles arguments");
  if (n_levels == 0) return 0;
  const double *ds, *dq;
  double* dout;
  if (int r = c.in(sorted, (size_t)n, &ds)) return r;
  if (int r = c.in(conf_levels, (size_t)n_levels, &dq)) return r;
  if (int r = c.out(out, (size_t)n_levels, &dout)) return r;
  hipLaunchKernelGGL(qt::k_interp_sorted, dim3((n_levels + 255) / 256), dim3(256), 0, h->stream, ds, n, dq, n_levels, dout);
  return c.done();
}

// ---- a16 over several ranks: the order statistics interp1d needs from a sample whose sorted shards live on N ranks
// (kernels and the argument in qt_ops.h; the two all-gathers in between are quantpy_amd/distributed.py's) -----------------
int qt_select_splitters(qt_handle_t* h, const double* sorted, long long n, long long stride, int P, double* splitters,
                        int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (n < 0 || stride < 1 || P < 1 || (n > 0 && !sorted) || !splitters) return fail(QT_ERR_ARG, "bad select_splitters arguments");
  const double* ds;
  double* dout;
  if (int r = c.in(sorted, (size_t)n, &ds)) return r;
  if (int r = c.out(splitters, (size_t)P, &dout)) return r;
  hipLaunchKernelGGL(qt::k_select_splitters, dim3((P + 255) / 256), dim3(256), 0, h->stream, ds, n, stride, P, dout);
  return c.done();
}

int qt_select_bracket(qt_handle_t* h, const double* splitters, int N, int P, const int64_t* sizes, long long stride,
                      long long n_total, const double* conf_levels, int L, uint64_t* lo_key, uint64_t* hi_key, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (N < 1 || P < 1 || L < 1 || stride < 1 || n_total < 0 || !splitters || !sizes || !conf_levels || !lo_key || !hi_key)
    return fail(QT_ERR_ARG, "bad select_bracket arguments");
  const double *dspl, *dq;
  const int64_t* dsz;
  uint64_t *dlo, *dhi;
  if (int r = c.in(splitters, (size_t)N * P, &dspl)) return r;
  if (int r = c.in(sizes, (size_t)N, &dsz)) return r;
  if (int r = c.in(conf_levels, (size_t)L, &dq)) return r;
  if (int r = c.out(lo_key, (size_t)L, &dlo)) return r;
  if (int r = c.out(hi_key, (size_t)L, &dhi)) return r;
  hipLaunchKernelGGL(qt::k_select_init, dim3((L + 255) / 256), dim3(256), 0, h->stream,
                     reinterpret_cast<unsigned long long*>(dlo), reinterpret_cast<unsigned long long*>(dhi), L);
  hipLaunchKernelGGL(qt::k_select_bracket, dim3((unsigned)(((size_t)N * P + 255) / 256)), dim3(256), 0, h->stream, dspl, N, P,
                     reinterpret_cast<const long long*>(dsz), stride, n_total, dq, L,
                     reinterpret_cast<unsigned long long*>(dlo), reinterpret_cast<unsigned long long*>(dhi));
  return c.done();
}

int qt_select_window(qt_handle_t* h, const double* sorted, long long n, const uint64_t* lo_key, const uint64_t* hi_key, int L,
                     int W, double* window, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (n < 0 || L < 1 || W < 1 || (n > 0 && !sorted) || !lo_key || !hi_key || !window)
    return fail(QT_ERR_ARG, "bad select_window arguments");
  const double* ds;
  const uint64_t *dlo, *dhi;
  double* dwin;
  const size_t wn = (size_t)L * (2 + W);
  if (int r = c.in(sorted, (size_t)n, &ds)) return r;
  if (int r = c.in(lo_key, (size_t)L, &dlo)) return r;
  if (int r = c.in(hi_key, (size_t)L, &dhi)) return r;
  if (int r = c.out(window, wn, &dwin)) return r;
  hipLaunchKernelGGL(qt::k_select_window, dim3(L), dim3(256), 0, h->stream, ds, n,
                     reinterpret_cast<const unsigned long long*>(dlo), reinterpret_cast<const unsigned long long*>(dhi), W, dwin);
  return c.done();
}

int qt_select_finish(qt_handle_t* h, const double* windows, int N, int L, int W, long long n_total, const double* conf_levels,
                     double* out, int32_t* overflow, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (N < 1 || L < 1 || W < 1 || n_total < 1 || !windows || !conf_levels || !out || !overflow)
    return fail(QT_ERR_ARG, "bad select_finish arguments");
  const double *dw, *dq;
  double* dout;
  int32_t* dfl;
  const size_t wn = (size_t)N * L * (2 + W);
  if (int r = c.in(windows, wn, &dw)) return r;
  if (int r = c.in(conf_levels, (size_t)L, &dq)) return r;
  if (int r = c.out(out, (size_t)L, &dout)) return r;
  if (int r = c.out(overflow, 1, &dfl)) return r;
  HIPCHK(hipMemsetAsync(dfl, 0, sizeof(int32_t), h->stream));
  size_t cap = (size_t)N * W;
  if (cap > 16000) cap = 16000;  // 128 KB of LDS; a larger union raises the overflow flag (heavy ties: take the merge path)
  const size_t lds = cap * sizeof(double) + ((size_t)N + 2) * sizeof(int);
  if (int r = launch(h, qt::k_select_finish, dim3(L), dim3(1024), lds, dw, N, L, W, (int)cap, n_total, dq, dout,
                     reinterpret_cast<int*>(dfl)))
    return r;
  return c.done();
}

// R sorted runs, concatenated in `runs` (lengths: a HOST array, the launch geometry depends on them) -> out sorted.
// Pairwise merge-path passes, ceil(log2 R) of them, ping-ponging between out and a scratch buffer.
int qt_merge_sorted(qt_handle_t* h, const double* runs, const int64_t* run_lengths, int R, double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (R < 1 || !run_lengths || !out) return fail(QT_ERR_ARG, "bad merge_sorted arguments");
  long long n = 0;
  for (int r = 0; r < R; ++r) {
    if (run_lengths[r] < 0) return fail(QT_ERR_ARG, "negative run length");
    n += run_lengths[r];
  }
  if (n == 0) return 0;
  if (!runs) return fail(QT_ERR_ARG, "bad merge_sorted arguments");
  const double* din;
  double* dout;
  if (int r = c.in(runs, (size_t)n, &din)) return r;
  if (int r = c.out(out, (size_t)n, &dout)) return r;
  std::vector<long long> len(run_lengths, run_lengths + R);
  int passes = 0;
  for (int m = R; m > 1; m = (m + 1) / 2) ++passes;
  if (passes == 0) {
    if (din != dout) HIPCHK(hipMemcpyAsync(dout, din, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  } else {
    HIPCHK(h->sort_alt.ensure((size_t)n * sizeof(double)));
    double* alt = h->sort_alt.as<double>();
    // the last pass must land in dout: choose the first destination accordingly (the source of pass 0 is din, read-only)
    const double* src = din;
    double* dst = (passes & 1) ? dout : alt;
    if (dst == src) return fail(QT_ERR_ARG, "qt_merge_sorted: out must not alias runs");
    constexpr int TILE = 8;
    for (int p = 0; p < passes; ++p) {
      std::vector<long long> next;
      long long at = 0;
      for (size_t r = 0; r < len.size(); r += 2) {
        const long long na = len[r], nb = r + 1 < len.size() ? len[r + 1] : 0;
        if (na + nb > 0) {
          const long long threads = (na + nb + TILE - 1) / TILE;
          hipLaunchKernelGGL(qt::k_merge_runs<TILE>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, src + at,
                             na, src + at + na, nb, dst + at);
        }
        next.push_back(na + nb);
        at += na + nb;
      }
      len.swap(next);
      src = dst;
      dst = (dst == dout) ? alt : dout;
    }
  }
  return c.done();
}

// ---- f2: stats.py:21-47 over a batch (MomentInterval, interval.py:59-110) ------------------------------------------------
// W = P^T P on the matrix cores ([M x rows] . [rows x M]), in h->gram
static int moment_gram(qt_handle_t* h, const double* dp, int rows, long long M, double** dW) {
  HIPCHK(h->gram.ensure((size_t)M * M * sizeof(double)));
  *dW = h->gram.as<double>();
  hipLaunchKernelGGL(qt::k_gemm<0>, dim3((unsigned)((M + 15) / 16), (unsigned)((M + 15) / 16)), dim3(64), 0, h->stream, (int)M, (int)M,
                     rows, dp, (int)M, 1, dp, (int)M, 0, *dW, (int)M);
  return 0;
}

// The moments of B trials from their frequencies in device memory, at any M (k_moment_cols, k_moment_finish).  The grid
// over W -- column blocks of whole settings (or pieces of one, K > 256) x runs of settings -- aims at about 1024 blocks
// per group of trials and at least 64 rows per block, and is a function of (S, K) alone.  256 trials per launch pair bound
// the workspace (40 B per block and trial, 8 S^2 ceil(K / 256) B per trial for K > 256).
static int moment_from_freq(qt_handle_t* h, const double* dfreq, int B, int S, int K, const double* dW, double n_trials,
                            double* dmean, double* dvar) {
  const int CB = qt::kMomentCols, T = qt::kMomentT;
  const int pieces = K <= CB ? 1 : (K + CB - 1) / CB, spb = K <= CB ? CB / K : 0;
  const int ncb = pieces == 1 ? (S + spb - 1) / spb : S * pieces;
  const int runs = std::min(S, std::max(1, 1024 / ncb));
  const int spr = std::min(S, std::max((S + runs - 1) / runs, (64 + K - 1) / K)), nrc = (S + spr - 1) / spr;
  const size_t nblk = (size_t)ncb * nrc, M = (size_t)S * K, per_q = pieces > 1 ? (size_t)S * S * pieces : 0;
  const int chunk = std::min(B, 256);
  HIPCHK(h->moment_part.ensure(chunk * nblk * 5 * sizeof(double)));
  HIPCHK(h->moment_qpart.ensure(chunk * per_q * sizeof(double)));
  double *part = h->moment_part.as<double>(), *qpart = h->moment_qpart.as<double>();
  for (int b0 = 0; b0 < B; b0 += chunk) {
    const int nb = std::min(chunk, B - b0);
    if (int r = launch(h, qt::k_moment_cols, dim3((nb + T - 1) / T, ncb, nrc), dim3(256), 0, dfreq + b0 * M, nb, S, K, dW, spb,
                       pieces, spr, part, qpart))
      return r;
    if (int r = launch(h, qt::k_moment_finish, dim3(nb), dim3(64), 0, (const double*)part, (int)nblk, (const double*)qpart, S,
                       pieces, n_trials, dmean + b0, dvar + b0))
      return r;
  }
  return 0;
}

static int moment_too_large(long long M) {
  return fail(QT_ERR_UNSUPPORTED, "the moment entries support up to %d POVM rows (got %lld: W = P^T P would take %.1f GiB)",
              qt::kMomentMaxRows, M, (double)M * (double)M * 8.0 / 1073741824.0);
}

int qt_moment_batch(qt_handle_t* h, const int64_t* counts, int B, int S, int K, const double* ns, const double* inv_matrix,
                    int rows, double n_trials, double* mean, double* var, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || S < 1 || K < 1 || rows < 1 || !(n_trials > 0.0) || !ns || !inv_matrix || (B > 0 && (!counts || !mean || !var)))
    return fail(QT_ERR_ARG, "bad moment_batch arguments");
  const long long M = (long long)S * K;
  if (M > qt::kMomentMaxRows) return moment_too_large(M);
  if (B == 0) return 0;
  const int64_t* dc;
  const double *dns, *dp;
  double *dmean, *dvar, *dW;
  if (int r = c.in(counts, (size_t)B * M, &dc)) return r;
  if (int r = c.in(ns, (size_t)S, &dns)) return r;
  if (int r = c.in(inv_matrix, (size_t)rows * M, &dp)) return r;
  if (int r = c.out(mean, (size_t)B, &dmean)) return r;
  if (int r = c.out(var, (size_t)B, &dvar)) return r;
  if (int r = moment_gram(h, dp, rows, M, &dW)) return r;
  if (M <= 8192) {  // f and U f of whole trials in LDS
    const int T = M <= 1024 ? 4 : 1;  // trials per workgroup
    if (int r = launch(h, T == 4 ? qt::k_moment_batch<4, 4> : qt::k_moment_batch<1, 32>, dim3((B + T - 1) / T), dim3(256),
                       (size_t)2 * T * M * sizeof(double), dc, B, S, K, dns, (const double*)dW, n_trials, dmean, dvar))
      return r;
  } else {
    const long long total = (long long)B * M;
    HIPCHK(h->moment_freq.ensure((size_t)total * sizeof(double)));
    double* dfreq = h->moment_freq.as<double>();
    if (int r = launch(h, qt::k_counts_to_freq, dim3(grid_for((size_t)total)), dim3(256), 0, dc, total, S, K, dns, dfreq)) return r;
    if (int r = moment_from_freq(h, dfreq, B, S, K, dW, n_trials, dmean, dvar)) return r;
  }
  return c.done();
}

int qt_moment_freq_batch(qt_handle_t* h, const double* freq, int B, int S, int K, const double* inv_matrix, int rows,
                         double n_trials, double* mean, double* var, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || S < 1 || K < 1 || rows < 1 || !(n_trials > 0.0) || !inv_matrix || (B > 0 && (!freq || !mean || !var)))
    return fail(QT_ERR_ARG, "bad moment_freq_batch arguments");
  const long long M = (long long)S * K;
  if (M > qt::kMomentMaxRows) return moment_too_large(M);
  if (B == 0) return 0;
  const double *df, *dp;
  double *dmean, *dvar, *dW;
  if (int r = c.in(freq, (size_t)B * M, &df)) return r;
  if (int r = c.in(inv_matrix, (size_t)rows * M, &dp)) return r;
  if (int r = c.out(mean, (size_t)B, &dmean)) return r;
  if (int r = c.out(var, (size_t)B, &dvar)) return r;
  if (int r = moment_gram(h, dp, rows, M, &dW)) return r;
  if (int r = moment_from_freq(h, df, B, S, K, dW, n_trials, dmean, dvar)) return r;
  return c.done();
}

// ---- f3: interval.py:268-335, the LPs of PolytopeStateInterval (qt_lp.h, qt_lp_large.h, qt_lp_xl.h) --------------------
// The LP entries: `name` for the messages, at most max_n variables, per_wg bytes of workspace per workgroup in `ws`, at
// most max_grid workgroups and ws_cap bytes of workspace in all.  The large entries refuse a workgroup's workspace
// above the cap (refuse_ws); the small one then runs one workgroup.
constexpr size_t kLpWsCap = (size_t)256 << 20;
// qt_lp_ineq_xl_batch: a workgroup holds 124 KB of LDS, so one runs per compute unit (256), each with 8 MB + 7 M doubles
constexpr long long kLpXlGrid = 256;
constexpr size_t kLpXlWsCap = (size_t)4 << 30;
using LpKernel = void (*)(const double*, int, int, const double*, int, const double*, int, double*, double*, int32_t*,
                          int32_t*, double*);
static int lp_ineq_entry(qt_handle_t* h, const char* name, int max_n, size_t per_wg, bool refuse_ws, long long max_grid,
                         size_t ws_cap, DevBuf qt_handle_t::*ws,
                         LpKernel kernel, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                         double* obj, double* x, int32_t* status, int32_t* iters, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!A || !C || !b || !obj || !status) return fail(QT_ERR_ARG, "%s: null array", name);
  if (N < 1 || M < N || O < 1 || R < 1) return fail(QT_ERR_ARG, "%s: bad sizes (M=%d N=%d O=%d R=%d)", name, M, N, O, R);
  if (N > max_n) return fail(QT_ERR_UNSUPPORTED, "%s supports up to %d variables (got %d)", name, max_n, N);
  const long long P = (long long)R * O;
  if (P > (1LL << 30)) return fail(QT_ERR_ARG, "%s: too many programs (%lld)", name, P);
  const double *dA, *dC, *db;
  double *dobj, *dx;
  int32_t *dst, *dit;
  if (int r = c.in(A, (size_t)M * N, &dA)) return r;
  if (int r = c.in(C, (size_t)O * N, &dC)) return r;
  if (int r = c.in(b, (size_t)R * M, &db)) return r;
  if (int r = c.out(obj, (size_t)P, &dobj)) return r;
  if (int r = c.out(x, (size_t)P * N, &dx)) return r;
  if (int r = c.out(status, (size_t)P, &dst)) return r;
  if (int r = c.out(iters, (size_t)P, &dit)) return r;
  // persistent workgroups: at most max_grid, and at most ws_cap of workspace (2048 and 256 MB for the two smaller
  // kernels: the large one takes about 0.6 MB each, about 400 workgroups)
  long long grid = P < max_grid ? P : max_grid;
  const long long by_ws = (long long)(ws_cap / per_wg);
  if (by_ws < 1 && refuse_ws)
    return fail(QT_ERR_UNSUPPORTED, "%s: M = %d needs more than %zu MB of workspace per program", name, M, ws_cap >> 20);
  if (grid > by_ws) grid = by_ws > 0 ? by_ws : 1;
  HIPCHK((h->*ws).ensure((size_t)grid * per_wg));
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(qt::kLpNT), 0, h->stream, dA, M, N, dC, O, db, R, dobj, dx, dst, dit,
                     (h->*ws).as<double>());
  return c.done(status, (int)P);
}

int qt_lp_ineq_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                     double* obj, double* x, int32_t* status, int32_t* iters, int flags) {
  return lp_ineq_entry(h, "qt_lp_ineq_batch", qt::kLpMaxN, qt::LpSmall::ws_doubles(M) * sizeof(double), false, 2048, kLpWsCap,
                       &qt_handle_t::lp_ws,
                       qt::k_lp_ineq, A, M, N, C, O, b, R, obj, x, status, iters, flags);
}

// The same programs for 65 ... 255 variables (qt_lp_large.h): the normal matrix lives in the workspace, not in LDS.
int qt_lp_ineq_large_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                           double* obj, double* x, int32_t* status, int32_t* iters, int flags) {
  return lp_ineq_entry(h, "qt_lp_ineq_large_batch", qt::kLgMaxN, qt::LpLarge::ws_doubles(M) * sizeof(double), true, 2048,
                       kLpWsCap, &qt_handle_t::lp_large_ws, qt::k_lp_ineq_large, A, M, N, C, O, b, R, obj, x, status, iters, flags);
}

// The same programs for up to 1023 variables (qt_lp_xl.h): the polytope of a five-qubit state.
int qt_lp_ineq_xl_batch(qt_handle_t* h, const double* A, int M, int N, const double* C, int O, const double* b, int R,
                        double* obj, double* x, int32_t* status, int32_t* iters, int flags) {
  return lp_ineq_entry(h, "qt_lp_ineq_xl_batch", qt::kXlMaxN, qt::LpXl::ws_doubles(M) * sizeof(double), true, kLpXlGrid,
                       kLpXlWsCap, &qt_handle_t::lp_xl_ws, qt::k_lp_ineq_xl, A, M, N, C, O, b, R, obj, x, status, iters, flags);
}

// The primitives of one of the three LP kernels, run once by one workgroup on the caller's vectors (k_lp_pieces): a test
// and diagnosis entry.  The workgroup's workspace slice and every output are filled with 0xFF bytes (NaN) before the launch.
static int lp_pieces_entry(qt_handle_t* h, Call& c, int kernel, const char* what, int max_n, size_t per_wg, bool refuse_ws,
                           size_t ws_cap, DevBuf& ws, const double* A, int M, int N, const double* w, const double* vm,
                           const double* vn, int p1, int mode, double* normal, double* factor, double* u, double* ax,
                           double* solved, int32_t* ok) {
  if (N > max_n) return fail(QT_ERR_UNSUPPORTED, "qt_lp_pieces: %s supports up to %d variables (got %d)", what, max_n, N);
  if (refuse_ws && per_wg > ws_cap)
    return fail(QT_ERR_UNSUPPORTED, "qt_lp_pieces: M = %d needs more than %zu MB of workspace per program", M, ws_cap >> 20);
  const size_t n = (size_t)N + (p1 ? 1 : 0);
  const double *dA, *dw, *dvm, *dvn;
  double *dnormal, *dfactor, *du, *dax, *dsolved;
  int32_t* dok;
  if (int r = c.in(A, (size_t)M * N, &dA)) return r;
  if (int r = c.in(w, (size_t)M, &dw)) return r;
  if (int r = c.in(vm, (size_t)M, &dvm)) return r;
  if (int r = c.in(vn, n, &dvn)) return r;
  if (int r = c.out(normal, n * n, &dnormal)) return r;
  if (int r = c.out(factor, n * n, &dfactor)) return r;
  if (int r = c.out(u, n, &du)) return r;
  if (int r = c.out(ax, (size_t)M, &dax)) return r;
  if (int r = c.out(solved, n, &dsolved)) return r;
  if (int r = c.out(ok, (size_t)1, &dok)) return r;
  HIPCHK(ws.ensure(per_wg));
  HIPCHK(hipMemsetAsync(ws.p, 0xFF, per_wg, h->stream));
  const struct {
    void* p;
    size_t bytes;
  } outs[] = {{dnormal, n * n * sizeof(double)}, {dfactor, n * n * sizeof(double)}, {du, n * sizeof(double)},
              {dax, (size_t)M * sizeof(double)}, {dsolved, n * sizeof(double)},     {dok, sizeof(int32_t)}};
  for (const auto& o : outs)
    if (o.p) HIPCHK(hipMemsetAsync(o.p, 0xFF, o.bytes, h->stream));
  qt::lp_pieces_launch(kernel, h->stream, dA, M, N, dw, dvm, dvn, p1, mode, dnormal, dfactor, du, dax, dsolved, dok,
                       ws.as<double>());
  return c.done();
}

int qt_lp_pieces(qt_handle_t* h, int kernel, const double* A, int M, int N, const double* w, const double* vm,
                 const double* vn, int p1, int mode, double* normal, double* factor, double* u, double* ax, double* solved,
                 int32_t* ok, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!A || !w || !vm || !vn) return fail(QT_ERR_ARG, "qt_lp_pieces: null array");
  if (N < 1 || M < N) return fail(QT_ERR_ARG, "qt_lp_pieces: bad sizes (M=%d N=%d)", M, N);
  if (kernel < 0 || kernel > 2 || (p1 != 0 && p1 != 1) || (mode != 0 && mode != 1) || (mode == 1 && p1))
    return fail(QT_ERR_ARG, "qt_lp_pieces: bad selector (kernel=%d p1=%d mode=%d; the rank test has no border)", kernel, p1, mode);
  if (kernel == 0)
    return lp_pieces_entry(h, c, 0, "k_lp_ineq", qt::kLpMaxN, qt::LpSmall::ws_doubles(M) * sizeof(double),
                            false, kLpWsCap, h->lp_ws, A, M, N, w, vm, vn, p1, mode, normal, factor, u, ax, solved, ok);
  if (kernel == 1)
    return lp_pieces_entry(h, c, 1, "k_lp_ineq_large", qt::kLgMaxN,
                            qt::LpLarge::ws_doubles(M) * sizeof(double), true, kLpWsCap, h->lp_large_ws, A, M, N, w, vm, vn, p1,
                            mode, normal, factor, u, ax, solved, ok);
  return lp_pieces_entry(h, c, 2, "k_lp_ineq_xl", qt::kXlMaxN, qt::LpXl::ws_doubles(M) * sizeof(double), true,
                          kLpXlWsCap, h->lp_xl_ws, A, M, N, w, vm, vn, p1, mode, normal, factor, u, ax, solved, ok);
}

// ---- f4: polytopes/utils.py:4-27, verification.py:9-78 over a batch of trials (qt_polytope.h) -------------------------
int qt_polytope_confidence(qt_handle_t* h, const int64_t* counts, long long B, int R, int K, const double* shots,
                           const double* deltas, int Q, double* conf, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || R < 1 || K < 1 || Q < 1 || !shots || (B > 0 && (!counts || !deltas || !conf)))
    return fail(QT_ERR_ARG, "qt_polytope_confidence: null array or bad sizes (B=%lld R=%d K=%d Q=%d)", B, R, K, Q);
  PolyPlan p;
  if (int r = poly_plan(R, K, &p)) return r;
  if (int r = poly_check_shots(h, c, shots, R, "qt_polytope_confidence")) return r;
  if (B == 0) return 0;
  const long long RK = (long long)R * K;
  if (B > kPolyMaxUnits / Q || B > kPolyMaxCounts / RK)
    return fail(QT_ERR_UNSUPPORTED, "qt_polytope_confidence: B x Q = %lld x %d (R K = %lld) is too large for one call", B, Q, RK);
  const long long units = B * Q, wave_grid = p.wave ? (units + 4 * (64 / p.TS) - 1) / (4 * (64 / p.TS)) : 0;
  const int64_t* dc;
  const double *dn, *dd;
  double* dconf;
  if (int r = c.in(counts, (size_t)(B * RK), &dc)) return r;
  if (int r = c.in(shots, (size_t)R, &dn)) return r;
  if (int r = c.in(deltas, (size_t)units, &dd)) return r;
  if (int r = c.out(conf, (size_t)units, &dconf)) return r;
  const int rl = poly_dispatch(
      p,
      [&] {
        return launch(h, qt::k_polytope_confidence_wave, dim3((unsigned)wave_grid), dim3(256), 0, dc, B, R, K, p.kshift, p.TS,
                      dn, dd, Q, dconf);
      },
      [&](auto nt, auto mode) {
        constexpr int NT = decltype(nt)::value, MODE = decltype(mode)::value;
        return launch(h, qt::k_polytope_confidence<NT, MODE>, dim3((unsigned)std::min(B, kPolyMaxGrid)), dim3(NT), p.lds, dc, B,
                      p.sh, dn, dd, Q, dconf);
      });
  if (rl) return rl;
  return c.done();
}

int qt_polytope_coverage(qt_handle_t* h, const int64_t* counts, long long B, int R, int K, const double* shots,
                         const double* levels, int L, const double* truth, int clip_b, double* deltas, uint8_t* hits,
                         long long* covered, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || R < 1 || K < 1 || L < 1 || !shots || !levels || (B > 0 && !counts) || (!deltas && !hits && !covered) ||
      ((hits || covered) && !truth))
    return fail(QT_ERR_ARG, "qt_polytope_coverage: null array or bad sizes (B=%lld R=%d K=%d L=%d)", B, R, K, L);
  PolyPlan p;
  if (int r = poly_plan(R, K, &p)) return r;
  if (int r = poly_check_shots(h, c, shots, R, "qt_polytope_coverage")) return r;
  if (B == 0) return 0;
  const long long RK = (long long)R * K;
  if (B > kPolyMaxUnits / L || B > kPolyMaxCounts / RK)
    return fail(QT_ERR_UNSUPPORTED, "qt_polytope_coverage: B x L = %lld x %d (R K = %lld) is too large for one call", B, L, RK);
  const long long units = B * L, wave_grid = p.wave ? (units + 4 * (64 / p.TS) - 1) / (4 * (64 / p.TS)) : 0;
  const int64_t* dc;
  const double *dn, *dl, *dt;
  double* dd;
  uint8_t* dh;
  long long* dcov = nullptr;
  if (int r = c.in(counts, (size_t)(B * RK), &dc)) return r;
  if (int r = c.in(shots, (size_t)R, &dn)) return r;
  if (int r = c.in(levels, (size_t)L, &dl)) return r;
  if (int r = c.in(truth, (size_t)RK, &dt)) return r;
  if (int r = c.out(deltas, (size_t)units, &dd)) return r;
  if (int r = c.out(hits, (size_t)units, &dh)) return r;
  if (covered) {
    if (int r = c.inout(covered, (size_t)L, &dcov)) return r;
    if (!dh) {
      HIPCHK(h->poly_ws.ensure((size_t)units));
      dh = h->poly_ws.as<uint8_t>();
    }
  }
  const int rl = poly_dispatch(
      p,
      [&] {
        return launch(h, qt::k_polytope_coverage_wave, dim3((unsigned)wave_grid), dim3(256), 0, dc, B, R, K, p.kshift, p.TS, dn,
                      dl, L, dt, clip_b, dd, dh);
      },
      [&](auto nt, auto mode) {
        constexpr int NT = decltype(nt)::value, MODE = decltype(mode)::value;
        return launch(h, qt::k_polytope_coverage<NT, MODE>, dim3((unsigned)std::min(B, kPolyMaxGrid)), dim3(NT), p.lds, dc, B,
                      p.sh, dn, dl, L, dt, clip_b, dd, dh);
      });
  if (rl) return rl;
  // one workgroup per level counts its column of hits and adds it to covered[l]: no contended atomics
  if (covered)
    if (int r = launch(h, qt::k_polytope_count, dim3(L), dim3(256), 0, (const uint8_t*)dh, B, L, dcov)) return r;
  return c.done();
}

// ---- a4 / a12 / a16 host side: state.py:109-114, the draws of experiment() (qt_sampler.h) ---------
int qt_legacy_multinomial(uint32_t* mt_key, int* mt_pos, long long rows, int period, const int64_t* n,
                          const double* pvals, int K, int64_t* out) {
  if (!mt_key || !mt_pos || !n || !pvals || (rows > 0 && !out) || rows < 0 || period < 1 || K < 1)
    return fail(QT_ERR_ARG, "bad legacy_multinomial arguments");
  if (*mt_pos < 0 || *mt_pos > 624) return fail(QT_ERR_ARG, "MT19937 position %d outside 0..624", *mt_pos);
  if (int r = check_pvals(period, K, n, pvals)) return r;
  qt_sampler::Mt19937 g{mt_key, *mt_pos};
  std::vector<qt_sampler::BinomialSetup> cache((size_t)period * K);
  for (long long r = 0; r < rows; ++r) {
    const int s = (int)(r % period);
    qt_sampler::legacy_multinomial(g, n[s], pvals + (size_t)s * K, K, out + (size_t)r * K, cache.data() + (size_t)s * K);
  }
  *mt_pos = g.pos;
  return 0;
}

int qt_device_multinomial(qt_handle_t* h, uint64_t seed, uint64_t first_row, long long rows, int period,
                          const int64_t* n, const double* pvals, int K, int64_t* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!n || !pvals || (rows > 0 && !out) || rows < 0 || period < 1 || K < 1)
    return fail(QT_ERR_ARG, "bad device_multinomial arguments");
  if (rows > (1LL << 40)) return fail(QT_ERR_UNSUPPORTED, "qt_device_multinomial draws at most 2^40 rows per call");
  if (!c.device())  // (device arrays are not read on the host)
    if (int r = check_pvals(period, K, n, pvals)) return r;
  if (rows == 0) return 0;
  const int64_t* dn;
  const double* dp;
  int64_t* dout;
  if (int r = c.in(n, (size_t)period, &dn)) return r;
  if (int r = c.in(pvals, (size_t)period * K, &dp)) return r;
  if (int r = c.out(out, (size_t)rows * K, &dout)) return r;
  // whole 64 x period blocks of rows per launch (a wavefront = one setting of 64 consecutive resamples); a launch covers at
  // most 2^30 threads -- HIP rejects grids of 2^32 threads and more -- so larger tables go out in chunks, each keyed by its
  // own first row: the table depends on (seed, global row) only
  const long long span = 64LL * period;
  const long long chunk_rows = (span >= (1LL << 30)) ? span : ((1LL << 30) / span) * span;
  for (long long r0 = 0; r0 < rows; r0 += chunk_rows) {
    const long long nr = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
    const long long threads = (nr + span - 1) / span * span;
    hipLaunchKernelGGL(qt_sampler::k_multinomial_rows, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, h->stream, seed,
                       first_row + (uint64_t)r0, nr, period, dn, dp, K, dout + (size_t)r0 * K);
  }
  return c.done();
}

void qt_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out) { qt_sampler::philox4x32_10(ctr, key, out); }

// ---- a5 for arbitrary matrices: routines.py:69-71 -------------------------------------------------
int qt_left_inverse(qt_handle_t* h, const double* A, int rows, int cols, int is_complex, double* out, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!A || !out || rows < 1 || cols < 1) return fail(QT_ERR_ARG, "bad left_inverse arguments");
  if (rows < cols) return fail(QT_ERR_SINGULAR, "matrix has fewer rows (%d) than columns (%d)", rows, cols);
  const int W = is_complex ? 2 : 1;
  const size_t nel = (size_t)rows * cols * W;
  const double* dA;
  double* dout;
  if (int r = c.in(A, nel, &dA)) return r;
  if (int r = c.out(out, nel, &dout)) return r;
  if (int r = is_complex ? enqueue_left_inverse<2>(h, dA, rows, cols, dout) : enqueue_left_inverse<1>(h, dA, rows, cols, dout))
    return r;
  int info = 0;
  HIPCHK(hipMemcpyAsync(&info, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (int r = c.done()) return r;
  if (c.device()) HIPCHK(hipStreamSynchronize(h->stream));  // (done() waits for host arrays only) the pivot report
  if (info != 0) return fail(QT_ERR_SINGULAR, "A^T A is singular (no pivot in column %d)", info - 1);
  return 0;
}

// ---- process tomography: qt_process.h -------------------------------------------------------------
int qt_process_setup(qt_handle_t* h, const double* in_states, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (!in_states) return fail(QT_ERR_ARG, "null in_states");
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "process tomography supports n_qubits 1..3 in this release");
  h->proc_set = false;
  if (int r = ensure_dense(h)) return r;
  const int d = h->d, D = h->D, M = h->M;
  const size_t C2 = (size_t)D * D, R = (size_t)D * M;
  ProcessState& ps = h->proc;
  ps.release();
  HIPCHK(ps.in_states.ensure((size_t)D * D * 2 * sizeof(double)));
  HIPCHK(ps.emats.ensure((size_t)M * D * 2 * sizeof(double)));
  if (int r = c.copy_in(ps.in_states.as<double>(), in_states, (size_t)D * D * 2)) return r;
  // E_m = sum_k A'[m][k] P_k  (process.py:204: Qobj(povm_bloch).matrix)
  if (int r = launch(h, qt::k_mat_from_bloch, dim3(grid_for((size_t)M * D)), dim3(256), 0, h->nq, h->povm.Aw.as<double>(), M,
                     ps.emats.as<double>()))
    return r;
  // n = 3 keeps the Kronecker-factored design matrix only (qt_process64.h): L = (V_S (x) V_P) Pi^T, L^+ = Pi (V_S^+ (x) V_P^+).
  // n = 2 builds the factors too where k_lifp16 can take them (qt_process.h): what qt_lifp_batch multiplies by; the dense
  // operators stay for qt_process_get_operators, 'pgdb' and the process chain.
  const bool factored = h->nq == 3;
  const bool factors = factored || (h->nq == 2 && M % 4 == 0 && (size_t)M * 32 * sizeof(double) <= 64 * 1024);
  int info = 0, finfo[2] = {0, 0};
  if (!factored) {
    HIPCHK(ps.lifp.ensure(R * C2 * 2 * sizeof(double)));
    HIPCHK(ps.pinv.ensure(R * C2 * 2 * sizeof(double)));
    HIPCHK(ps.pinvT.ensure(R * C2 * 2 * sizeof(double)));
    double *lifp = ps.lifp.as<double>(), *pinv = ps.pinv.as<double>(), *pinvT = ps.pinvT.as<double>();
    if (int r = launch(h, qt::k_lifp_rows, dim3(grid_for(R * C2)), dim3(256), 0, d, M, ps.in_states.as<double>(),
                       ps.emats.as<double>(), lifp))
      return r;
    if (int r = enqueue_left_inverse<2>(h, lifp, (int)R, (int)C2, pinv)) return r;
    if (int r = launch_transpose<2>(h, pinv, (int)C2, (int)R, pinvT)) return r;
    if (h->nq == 2) {  // the batched GEMM of qt_lifp_batch reads the left inverse in row-major Choi order
      HIPCHK(ps.pinvR.ensure(R * C2 * 2 * sizeof(double)));
      if (int r = launch(h, qt::k_choi_order_rows, dim3(grid_for(R * C2)), dim3(256), 0, pinvT, R, D, ps.pinvR.as<double>()))
        return r;
    }
    HIPCHK(hipMemcpyAsync(&info, h->info.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  }
  if (factors)  // the permuted operand of k_lifp64 / k_lifp16 (the matrix-core paths of qt_lifp_batch) wants M % 4 == 0
    if (int r = enqueue_factors(h, M % 4 ? 0 : (factored ? 4 : 1), finfo)) return r;
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  if (info != 0) return fail(QT_ERR_SINGULAR, "process design matrix is rank deficient (column %d): input states x POVM not complete", info - 1);
  if (factored && finfo[0] != 0) return fail(QT_ERR_SINGULAR, "input states do not span the operator space (column %d)", finfo[0] - 1);
  if (factored && finfo[1] != 0) return fail(QT_ERR_SINGULAR, "POVM is not informationally complete (column %d)", finfo[1] - 1);
  ps.factored = factored;
  ps.factors = factors && finfo[0] == 0 && finfo[1] == 0;
  ps.perm = ps.factors && M % 4 == 0;
  if (factors && !ps.factors)  // n = 2 goes on with the dense form alone (cannot happen when the Kronecker product has full rank)
    for (DevBuf* b : {&ps.vs_pinv, &ps.vp_pinv, &ps.vp_pinvT, &ps.vp_perm}) b->release();
  h->proc_set = true;
  return 0;
}

int qt_process_get_operators(qt_handle_t* h, double* lifp_oper, double* lifp_oper_inv, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (h->proc.factored)
    return fail(QT_ERR_UNSUPPORTED, "at n = 3 the design matrix is kept Kronecker-factored (qt_process_get_factors); its dense "
                                    "form would be 2 x 906 MB");
  const size_t n = (size_t)h->D * h->M * h->D * h->D * 2;
  if (int r = c.copy_out(lifp_oper, h->proc.lifp.as<const double>(), n)) return r;
  if (int r = c.copy_out(lifp_oper_inv, h->proc.pinv.as<const double>(), n)) return r;
  return c.done();
}

int qt_process_prefer_dense(qt_handle_t* h, int on) {
  QT_ENTER(h);
  h->proc_dense = on != 0;
  return 0;
}

int qt_process_get_factors(qt_handle_t* h, double* vs_pinv, double* vp_pinv, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (!h->proc.factors)
    return fail(QT_ERR_UNSUPPORTED, "this set-up keeps the dense operator only (n = 1, or a POVM with M % 4 != 0 at n = 2): "
                                    "qt_process_get_operators");
  if (int r = c.copy_out(vs_pinv, h->proc.vs_pinv.as<const double>(), (size_t)h->D * h->D * 2)) return r;
  if (int r = c.copy_out(vp_pinv, h->proc.vp_pinv.as<const double>(), (size_t)h->D * h->M * 2)) return r;
  return c.done();
}

int qt_lifp_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, double* choi, int32_t* iters, int32_t* status,
                  int flags) {
  return lifp_batch_impl(h, false, counts, B, cptp, nullptr, 1, choi, nullptr, iters, status, flags, __func__);
}

int qt_lifp_dist_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, const double* centre, double* choi,
                       double* dist, int32_t* iters, int32_t* status, int flags) {
  return lifp_batch_impl(h, true, counts, B, cptp, centre, 1, choi, dist, iters, status, flags, __func__);
}

int qt_lifp_dist_group_batch(qt_handle_t* h, const int64_t* counts, int B, int cptp, const double* centres, int G, double* choi,
                             double* dist, int32_t* iters, int32_t* status, int flags) {
  return lifp_batch_impl(h, true, counts, B, cptp, centres, G, choi, dist, iters, status, flags, __func__);
}

// The resampling table of the process bootstrap: output states (k_choi_apply), their Bloch vectors and the Born rule by the
// kernels of qt_bloch_from_mat / qt_born_probs on the handle's workspace, then the clip np.random.multinomial's pvals get.
int qt_process_born_probs(qt_handle_t* h, const double* choi, int G, double* p, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (int r = need_povm(h)) return r;
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (G < 0 || (G > 0 && (!choi || !p))) return fail(QT_ERR_ARG, "bad process_born_probs arguments");
  if (G == 0) return 0;
  const int D = h->D, M = h->M;
  if ((long long)G * D > INT32_MAX / 2) return fail(QT_ERR_ARG, "batch too large");
  const int B = G * D;  // output states
  const size_t ne2 = (size_t)D * D * 2, nmat = (size_t)B * D * 2, np = (size_t)B * M;
  const double* dchoi;
  double* dp;
  if (int r = c.in(choi, (size_t)G * ne2, &dchoi)) return r;
  if (int r = c.out(p, np, &dp)) return r;
  HIPCHK(h->born_ws.ensure((nmat + (size_t)B * D) * sizeof(double)));
  double *mat = h->born_ws.as<double>(), *bloch = mat + nmat;
  if (int r = launch(h, qt::k_choi_apply, dim3(grid_for((size_t)B * D)), dim3(256), 0, h->d, dchoi, h->proc.in_states.as<double>(),
                     (size_t)B * D, mat))
    return r;
  if (int r = launch(h, qt::k_bloch_from_mat, dim3(grid_for((size_t)B * D)), dim3(256), 0, h->nq, (const double*)mat, B, bloch))
    return r;
  if (int r = born_launch(h, bloch, B, dp)) return r;
  if (int r = launch(h, qt::k_clip01, dim3(grid_for(np)), dim3(256), 0, dp, np)) return r;
  return c.done();
}

int qt_pgdb_batch(qt_handle_t* h, const int64_t* counts, int B, int n_iter, double tol, int stop_rule, double* choi,
                  int32_t* iters, int32_t* status, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (B < 0 || (B > 0 && (!counts || !choi))) return fail(QT_ERR_ARG, "bad pgdb_batch arguments");
  if (stop_rule != 0 && stop_rule != 1) return fail(QT_ERR_ARG, "stop_rule must be 0 (reference) or 1 (converged)");
  if (n_iter < 0) return fail(QT_ERR_ARG, "n_iter must be >= 0");
  if (B == 0) return 0;
  const int D = h->D, M = h->M;
  const int64_t* dc;
  double* dchoi;
  int32_t *dit, *dst;
  if (int r = c.in(counts, (size_t)B * D * M, &dc)) return r;
  if (int r = c.out(choi, (size_t)B * D * D * 2, &dchoi)) return r;
  if (int r = c.out(iters, (size_t)B, &dit)) return r;
  if (int r = c.out(status, (size_t)B, &dst)) return r;
  if (h->proc.factored) {  // n = 3: three launches per iteration over the batch, loop state on the device (qt_process64.h)
    using S = qt::Pgdb64;
    if (int r = pgdb64_scratch(h, B)) return r;
    int32_t *state = h->ws_act.as<int32_t>(), *n_active = state + (size_t)B * 4;
    if (int r = launch(h, qt::k_pgdb64_init, dim3(B), dim3(256), 0, B, dchoi, state, dit, dst, n_active)) return r;
    for (int it = 0; it < n_iter; ++it) {
      if (int r = pgdb64_trial(h, dc, B, dchoi)) return r;
      if (int r = launch(h, qt::k_pgdb64_step, dim3(B), dim3(S::NT), S::kLdsBytes, dc, B, M, h->proc.in_states.as<double>(),
                         h->proc.emats.as<double>(), h->ws_f.as<double>(), n_iter, tol, stop_rule, dchoi, state,
                         h->ws_x.as<double>(), dit, dst, n_active))
        return r;
      int left = 0;
      HIPCHK(hipMemcpyAsync(&left, n_active, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      if (left <= 0) break;
    }
    HIPCHK(hipGetLastError());
    return c.done(status, B);
  }
  const size_t dyn = (size_t)4 * D * M * sizeof(double);
  if (dyn > 32 * 1024) return fail(QT_ERR_UNSUPPORTED, "POVM has too many rows for the process kernel");
  if (int r = launch(h, D == 4 ? qt::k_pgdb_batch<4> : qt::k_pgdb_batch<16>, dim3(B),
                     dim3(D == 4 ? qt::ProcWG<4>::NT : qt::ProcWG<16>::NT), dyn, dc, B, M, h->proc.lifp.as<double>(), n_iter, tol,
                     stop_rule, dchoi, dit, dst))
    return r;
  return c.done(status, B);
}

int qt_pgdb_pieces(qt_handle_t* h, const int64_t* counts, int B, const double* choi_in, double* probas, double* grad,
                   double* projected, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (B < 0 || (B > 0 && (!counts || !choi_in))) return fail(QT_ERR_ARG, "bad pgdb_pieces arguments");
  if (!h->proc.factored) return fail(QT_ERR_UNSUPPORTED, "qt_pgdb_pieces inspects the factored (n = 3) iteration");
  if (B == 0) return 0;
  using S = qt::Pgdb64;
  const int D = h->D, M = h->M, R = D * M;
  const size_t ne2 = (size_t)D * D * 2;
  const int64_t* dc;
  const double* dcur;
  if (int r = c.in(counts, (size_t)B * R, &dc)) return r;
  if (int r = c.in(choi_in, (size_t)B * ne2, &dcur)) return r;
  if (int r = pgdb64_scratch(h, B)) return r;
  HIPCHK(hipMemsetAsync(h->ws_act.p, 0, ((size_t)B * 4 + 4) * sizeof(int32_t), h->stream));  // no process has stopped
  if (int r = pgdb64_trial(h, dc, B, dcur)) return r;
  HIPCHK(hipGetLastError());
  // p and g of every process's block, strided by the block, into the caller's dense arrays
  const S::Ws ws(h->ws_x.as<double>(), 0, M);
  const size_t pitch = S::ws_doubles(M) * sizeof(double);
  if (probas)
    HIPCHK(hipMemcpy2DAsync(probas, (size_t)R * sizeof(double), ws.p(), pitch, (size_t)R * sizeof(double), B, c.to_caller(),
                            h->stream));
  if (grad) HIPCHK(hipMemcpy2DAsync(grad, ne2 * sizeof(double), ws.g(), pitch, ne2 * sizeof(double), B, c.to_caller(), h->stream));
  if (int r = c.copy_out(projected, h->ws_f.as<const double>(), (size_t)B * ne2)) return r;
  return c.done();
}

int qt_mhmc_process(qt_handle_t* h, const int64_t* counts, int C, const double* choi_init, const double* deltas,
                    const double* uniforms, int T, double step, double* chain, int32_t* accepted, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (C < 0 || T < 0 || (C > 0 && T > 0 && (!counts || !choi_init || !deltas || !uniforms || !chain || !accepted)))
    return fail(QT_ERR_ARG, "bad mhmc_process arguments");
  if (C == 0 || T == 0) return 0;
  const int D = h->D, M = h->M;
  const size_t ne = (size_t)D * D;
  const int64_t* dc;
  const double *dx, *dd, *du;
  double* dch;
  int32_t* dacc;
  if (int r = c.in(counts, (size_t)C * D * M, &dc)) return r;
  if (int r = c.in(choi_init, (size_t)C * ne * 2, &dx)) return r;
  if (int r = c.in(deltas, (size_t)C * T * ne, &dd)) return r;
  if (int r = c.in(uniforms, (size_t)C * T, &du)) return r;
  if (int r = c.out(chain, (size_t)C * T * ne * 2, &dch)) return r;
  if (int r = c.out(accepted, (size_t)C * T, &dacc)) return r;
  if (h->proc.factored) {  // n = 3: four launches per step, the chain's state stays on the device (qt_process64.h)
    const int nt = qt::Fwd64::tiles(M);
    HIPCHK(h->ws_x.ensure(((size_t)C + (size_t)C * nt) * sizeof(double)));  // the points' NLLs and their pieces per row tile
    HIPCHK(h->ws_g.ensure((size_t)C * ne * 2 * sizeof(double)));     // proposals before the projection
    HIPCHK(h->ws_f.ensure((size_t)C * ne * 2 * sizeof(double)));     // ... and after it
    HIPCHK(h->hess.ensure((size_t)C * ne * 2 * sizeof(double)));     // the chains' current points
    double *fcur = h->ws_x.as<double>(), *fpart = fcur + C, *x = h->hess.as<double>();
    double *trial = h->ws_g.as<double>(), *proj = h->ws_f.as<double>();
    const double *vs = h->proc.in_states.as<double>(), *vp = h->proc.emats.as<double>(), *none = nullptr;
    HIPCHK(hipMemcpyAsync(x, dx, (size_t)C * ne * 2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    // the model and the NLL of a point: C x ceil(M / 16) workgroups on the matrix cores (k_fwd64_nll), then the accept test
    if (int r = launch(h, qt::k_fwd64_nll, dim3(C * nt), dim3(256), qt::Fwd64::kLdsBytes, dc, C, M, vs, vp, x, none, 0, fpart))
      return r;
    if (int r = launch(h, qt::k_mhmc64_decide, dim3(C), dim3(256), 0, C, nt, T, -1, fpart, none, du, x, fcur, dch, dacc)) return r;
    for (int t = 0; t < T; ++t) {
      if (int r = launch(h, qt::k_mhmc64_propose, dim3(C), dim3(256), 0, C, T, t, step, x, dd, trial)) return r;
      if (int r = project(h, trial, C, 0, 1000, 1e-12, proj, nullptr, nullptr)) return r;
      if (int r = launch(h, qt::k_fwd64_nll, dim3(C * nt), dim3(256), qt::Fwd64::kLdsBytes, dc, C, M, vs, vp, x, proj, 1, fpart))
        return r;
      if (int r = launch(h, qt::k_mhmc64_decide, dim3(C), dim3(256), 0, C, nt, T, t, fpart, proj, du, x, fcur, dch, dacc)) return r;
    }
    HIPCHK(hipGetLastError());
    return c.done();
  }
  const size_t dyn = (size_t)2 * D * M * sizeof(double);
  if (dyn > 32 * 1024) return fail(QT_ERR_UNSUPPORTED, "POVM has too many rows for the process kernel");
  if (int r = launch(h, D == 4 ? qt::k_mhmc_process<4> : qt::k_mhmc_process<16>, dim3(C),
                     dim3(D == 4 ? qt::ProcWG<4>::NT : qt::ProcWG<16>::NT), dyn, dc, C, M, h->proc.lifp.as<double>(), dx, dd, du, T,
                     step, dch, dacc))
    return r;
  return c.done();
}

// What the entries of the process chain whose numbers are drawn on the device (qt_sampler::mhmc_draw with vector length
// D^2) ask of the handle: n <= 2, the one-workgroup chain of qt_process.h, then a POVM and the input states
static int mhmc_process_ready(qt_handle_t* h, const char* fn) {
  if (h->nq > 2)
    return fail(QT_ERR_UNSUPPORTED, "%s supports n_qubits 1..2 (got %d): the device-drawn process chain has no n = 3 kernel", fn,
                h->nq);
  if (int r = need_povm(h)) return r;
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  return 0;
}

int qt_mhmc_process_draws(qt_handle_t* h, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T,
                          double* deltas, double* uniforms, int flags) {
  QT_ENTER(h);
  if (int r = mhmc_process_ready(h, "qt_mhmc_process_draws")) return r;
  return mhmc_draws_call(h, "qt_mhmc_process_draws", h->D * h->D, seed, first_chain, C, first_step, T, deltas, uniforms, flags);
}

// qt_mhmc_process_hits and qt_mhmc_process_metric_hits (mhmc_hits_call): one workgroup per chain; the infidelity's roots
// of the C centres into metric_ws first, by the set-up kernel of qt_metric_dist_dim at dim = D
static int mhmc_process_hits_impl(qt_handle_t* h, const char* fn, bool hs, int metric, const int64_t* counts, int C,
                                  const double* centres, const double* choi_init, const double* thresholds, uint64_t seed,
                                  uint64_t first_chain, int burn_steps, int n_points, int thinning, double step, int64_t* hits,
                                  int64_t* accepted, double* dist, int flags) {
  auto refuse = [&](MhmcHitsElems& n) {
    const size_t ne2 = (size_t)h->D * h->D * 2;
    n = {(size_t)h->D * h->M, ne2, ne2};
    return mhmc_process_ready(h, fn);
  };
  auto launch_chains = [&](const MhmcHitsArgs& a) {
    const int D = h->D, M = h->M;
    const size_t dyn = (size_t)2 * D * M * sizeof(double);
    if (dyn > 32 * 1024) return fail(QT_ERR_UNSUPPORTED, "POVM has too many rows for the process kernel");
    const dim3 block(D == 4 ? qt::ProcWG<4>::NT : qt::ProcWG<16>::NT);
    const double *lifp = h->proc.lifp.as<double>(), *dcen = a.centres;
    if (hs)
      return launch(h, D == 4 ? qt::k_mhmc_process_hits<4> : qt::k_mhmc_process_hits<16>, dim3(C), block, dyn, a.counts, C, M, lifp,
                    a.init, dcen, a.thresholds, seed, first_chain, a.burn_steps, a.n_points, a.thinning, step, a.hits, a.accepted,
                    a.dist);
    if (metric == QT_METRIC_INFIDELITY) {
      HIPCHK(h->metric_ws.ensure((size_t)C * D * D * 2 * sizeof(double)));
      double* roots = h->metric_ws.as<double>();
      using S2 = qt::Small<2>;
      if (int r = D == 4 ? launch(h, qt::k_psd_sqrt<2>, dim3((C + S2::TPB - 1) / S2::TPB), dim3(S2::NT), 0, dcen, C, h->jtol2, roots)
                         : launch(h, qt::k_psd_sqrt_dim<16>, dim3(C), dim3(qt::MetricDim<16>::NT), 0, dcen, C, h->jtol2, roots))
        return r;
      dcen = roots;
    }
    auto kernel = metric == QT_METRIC_TRACE
                      ? (D == 4 ? qt::k_mhmc_process_metric_hits<4, qt::kMetricTrace> : qt::k_mhmc_process_metric_hits<16, qt::kMetricTrace>)
                      : (D == 4 ? qt::k_mhmc_process_metric_hits<4, qt::kMetricInfidelity>
                                : qt::k_mhmc_process_metric_hits<16, qt::kMetricInfidelity>);
    return launch(h, kernel, dim3(C), block, dyn, a.counts, C, M, lifp, a.init, dcen, a.thresholds, seed, first_chain, a.burn_steps,
                  a.n_points, a.thinning, step, h->jtol2, a.hits, a.accepted, a.dist);
  };
  return mhmc_hits_call(h, fn, hs, metric, counts, C, centres, choi_init, thresholds, burn_steps, n_points, thinning, hits, accepted,
                        dist, flags, refuse, launch_chains);
}

int qt_mhmc_process_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* choi_init,
                         const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                         int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags) {
  return mhmc_process_hits_impl(h, "qt_mhmc_process_hits", true, 0, counts, C, centres, choi_init, thresholds, seed, first_chain,
                                burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_mhmc_process_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                const double* choi_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                                double* dist, int flags) {
  return mhmc_process_hits_impl(h, "qt_mhmc_process_metric_hits", false, metric, counts, C, centres, choi_init, thresholds, seed,
                                first_chain, burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_cptp_project_batch(qt_handle_t* h, const double* choi_in, int B, int mode, int n_iter, double tol, double* choi_out,
                          int32_t* iters, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (B < 0 || (B > 0 && (!choi_in || !choi_out))) return fail(QT_ERR_ARG, "bad cptp_project arguments");
  if (mode < 0 || mode > 2) return fail(QT_ERR_ARG, "mode must be 0 (CPTP), 1 (TP) or 2 (CP)");
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "process tomography supports n_qubits 1..3 in this release");
  if (B == 0) return 0;
  const int D = h->D;
  const double* din;
  double* dout;
  int32_t* dit;
  if (int r = c.in(choi_in, (size_t)B * D * D * 2, &din)) return r;
  if (int r = c.out(choi_out, (size_t)B * D * D * 2, &dout)) return r;
  if (int r = c.out(iters, (size_t)B, &dit)) return r;
  if (int r = project(h, din, B, mode, n_iter, tol, dout, dit, nullptr)) return r;
  return c.done();
}

// ---- the chain coverage study at n = 4, 5 (qt_mhmc_state_large.h)
// qt_mhmc_draws with the vector length given: any handle, no POVM
int qt_mhmc_draws_dim(qt_handle_t* h, int dim, uint64_t seed, uint64_t first_chain, int C, uint32_t first_step, int T,
                      double* deltas, double* uniforms, int flags) {
  QT_ENTER(h);
  if (dim < 2 || dim > 4096 || (dim & 1)) return fail(QT_ERR_ARG, "qt_mhmc_draws_dim: dim %d (even, 2 .. 4096)", dim);
  return mhmc_draws_call(h, "qt_mhmc_draws_dim", dim, seed, first_chain, C, first_step, T, deltas, uniforms, flags);
}

// qt_mhmc_state_large_hits and qt_mhmc_state_large_metric_hits (mhmc_hits_call), n = 4, 5: one workgroup per chain on the
// plan of qt_mhmc_state at these sizes, the infidelity's roots of the C centres by k_psd_sqrt_dim into metric_ws first, as
// metric_dim has them.  (These stand behind every older entry: the kernel templates are instantiated, and their device code
// laid out, in the order in which this file first names them, so the kernels that were here before stay where they were.)
static int mhmc_state_hits_large(qt_handle_t* h, const char* fn, bool hs, int metric, const int64_t* counts, int C, const double* centres,
                                 const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                 int burn_steps, int n_points, int thinning, double step, int64_t* hits, int64_t* accepted,
                                 double* dist, int flags) {
  auto refuse = [&](MhmcHitsElems& n) {
    if (h->nq <= 3)
      return fail(QT_ERR_UNSUPPORTED, "%s supports n_qubits 4, 5 (got %d): the entry for n <= 3 is %s", fn, h->nq,
                  hs ? "qt_mhmc_state_hits" : "qt_mhmc_state_metric_hits");
    n = {(size_t)h->M, (size_t)h->D * 2, (size_t)h->D};
    return need_povm(h);
  };
  auto launch_chains = [&](const MhmcHitsArgs& a) {
    return by_nq(h, [&](auto nq) {
      constexpr int NQ = decltype(nq)::value;
      if constexpr (NQ >= 4) {
        using S = qt::Large<NQ>;
        const Plan p = povm_plan<NQ>(h, C);
        if (hs)
          return launch(h, qt::k_mhmc_state_large_hits<NQ>, p, p.pv, a.counts, C, a.centres, a.init, a.thresholds, seed,
                        first_chain, a.burn_steps, a.n_points, a.thinning, step, a.hits, a.accepted, a.dist);
        if (metric == QT_METRIC_TRACE)
          return launch(h, qt::k_mhmc_state_large_metric_hits<NQ, qt::kMetricTrace>, p, p.pv, a.counts, C, a.centres, a.init,
                        a.thresholds, seed, first_chain, a.burn_steps, a.n_points, a.thinning, step, a.hits, a.accepted, a.dist);
        HIPCHK(h->metric_ws.ensure((size_t)C * S::D * 2 * sizeof(double)));
        double* roots = h->metric_ws.as<double>();
        if (int r = launch(h, qt::k_psd_sqrt_dim<S::d>, dim3(C), dim3(S::NT), 0, a.centres, C, h->jtol2, roots)) return r;
        return launch(h, qt::k_mhmc_state_large_metric_hits<NQ, qt::kMetricInfidelity>, p, p.pv, a.counts, C,
                      static_cast<const double*>(roots), a.init, a.thresholds, seed, first_chain, a.burn_steps, a.n_points,
                      a.thinning, step, a.hits, a.accepted, a.dist);
      } else {
        return 0;  // (refused above)
      }
    });
  };
  return mhmc_hits_call(h, fn, hs, metric, counts, C, centres, x_init, thresholds, burn_steps, n_points, thinning, hits, accepted,
                        dist, flags, refuse, launch_chains);
}

int qt_mhmc_state_large_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* x_init,
                             const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                             int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags) {
  return mhmc_state_hits_large(h, "qt_mhmc_state_large_hits", true, 0, counts, C, centres, x_init, thresholds, seed, first_chain,
                               burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_mhmc_state_large_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                    const double* x_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                    int burn_steps, int n_points, int thinning, double step, int64_t* hits,
                                    int64_t* accepted, double* dist, int flags) {
  return mhmc_state_hits_large(h, "qt_mhmc_state_large_metric_hits", false, metric, counts, C, centres, x_init, thresholds, seed,
                               first_chain, burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

// ---- the chain coverage study of three-qubit channels (qt_mhmc_process64.h)
// qt_mhmc_process_large_hits and qt_mhmc_process_large_metric_hits (mhmc_hits_call), n = 3: the launch family of
// qt_mhmc_process with the draws inside the propose and decide kernels, in slices of chains (QT_OPT_MHMC_PROCESS_SLICE)
// that bound the workspaces; no host synchronisation inside a slice, none between slices either.  Per chain of a slice:
// the current point (hess), the trial (ws_g) and its projection (ws_f) at 64 KB each, the projection's workspace
// (proc_ws, Proc64::kWsComplex), the NLL and its tile partials (ws_x) and, metric entry, the parked state and its distance
// (mhmc_parked).  The infidelity's roots of all C centres are made once per call (metric_ws), as metric_dim64 makes them.
static int mhmc_process_large_hits_impl(qt_handle_t* h, const char* fn, bool hs, int metric, const int64_t* counts, int C,
                                        const double* centres, const double* choi_init, const double* thresholds,
                                        uint64_t seed, uint64_t first_chain, int burn_steps, int n_points, int thinning,
                                        double step, int64_t* hits, int64_t* accepted, double* dist, int flags) {
  auto refuse = [&](MhmcHitsElems& n) {
    if (h->nq != 3)
      return fail(QT_ERR_UNSUPPORTED, "%s supports n_qubits 3 (got %d): the entry for n <= 2 is %s", fn, h->nq,
                  hs ? "qt_mhmc_process_hits" : "qt_mhmc_process_metric_hits");
    const size_t ne2 = (size_t)h->D * h->D * 2;
    n = {(size_t)h->D * h->M, ne2, ne2};
    if (int r = need_povm(h)) return r;
    if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
    return 0;
  };
  auto launch_chains = [&](const MhmcHitsArgs& a) {
    if (!h->proc.factored) return fail(QT_ERR_STATE, "%s: qt_process_setup left no factored operator", fn);
    using K = qt::Mhmc64;
    using W = qt::MetricDim64;
    const int M = h->M, nt = qt::Fwd64::tiles(M);
    const size_t ne2 = (size_t)K::NE * 2;
    const int slice = h->mhmc_process_slice > 0 ? h->mhmc_process_slice : 1024;
    const int ns = C < slice ? C : slice;  // the chains of the largest slice
    HIPCHK(h->ws_x.ensure(((size_t)ns + (size_t)ns * nt) * sizeof(double)));
    HIPCHK(h->ws_g.ensure((size_t)ns * ne2 * sizeof(double)));
    HIPCHK(h->ws_f.ensure((size_t)ns * ne2 * sizeof(double)));
    HIPCHK(h->hess.ensure((size_t)ns * ne2 * sizeof(double)));
    if (!hs) HIPCHK(h->mhmc_parked.ensure(((size_t)ns * ne2 + (size_t)ns) * sizeof(double)));
    double *fcur = h->ws_x.as<double>(), *fpart = fcur + ns, *x = h->hess.as<double>();
    double *trial = h->ws_g.as<double>(), *proj = h->ws_f.as<double>();
    double *parked = hs ? nullptr : h->mhmc_parked.as<double>(), *value = hs ? nullptr : parked + (size_t)ns * ne2;
    const double *vs = h->proc.in_states.as<double>(), *vp = h->proc.emats.as<double>(), *none = nullptr;
    const double* dcen = a.centres;
    if (!hs && metric == QT_METRIC_INFIDELITY) {
      HIPCHK(h->metric_ws.ensure((size_t)C * ne2 * sizeof(double)));
      double* roots = h->metric_ws.as<double>();
      if (int r = launch(h, qt::k_psd_sqrt_dim64, dim3(C), dim3(W::NT), W::kLdsBytes, a.centres, C, h->jtol2, roots)) return r;
      dcen = roots;
    }
    HIPCHK(hipMemsetAsync(a.hits, 0, (size_t)C * sizeof(int64_t), h->stream));
    HIPCHK(hipMemsetAsync(a.accepted, 0, (size_t)C * sizeof(int64_t), h->stream));
    const uint32_t total = a.burn_steps + a.n_points * a.thinning;  // (< 2^32 - 1: checked by mhmc_hits_call)
    for (int b0 = 0; b0 < C; b0 += slice) {
      const int nb = C - b0 < slice ? C - b0 : slice;
      const uint64_t gc0 = first_chain + (uint64_t)b0;
      const int64_t* dc = a.counts + (size_t)b0 * K::DC * M;
      const double *cen = dcen + (size_t)b0 * ne2, *thr = a.thresholds + b0;
      int64_t *dh = a.hits + b0, *da = a.accepted + b0;
      double* dd = a.dist ? a.dist + (size_t)b0 * a.n_points : nullptr;
      HIPCHK(hipMemcpyAsync(x, a.init + (size_t)b0 * ne2, (size_t)nb * ne2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
      // the NLL of the starting points, as qt_mhmc_process takes it (t = -1: no table is read)
      if (int r = launch(h, qt::k_fwd64_nll, dim3(nb * nt), dim3(256), qt::Fwd64::kLdsBytes, dc, nb, M, vs, vp, x, none, 0, fpart))
        return r;
      if (int r = launch(h, qt::k_mhmc64_decide, dim3(nb), dim3(256), 0, nb, nt, 0, -1, fpart, none, none, x, fcur,
                         (double*)nullptr, (int32_t*)nullptr))
        return r;
      uint32_t kept = 0, to_keep = 0;  // to_keep: steps until the next kept one (mhmc_process_hits_body)
      for (uint32_t j = 0; j < total; ++j) {
        const bool post = j >= a.burn_steps, keep = post && to_keep == 0;
        if (int r = launch(h, qt::k_mhmc64_propose_draw, dim3(nb), dim3(K::NT), 0, nb, seed, gc0, j, step, x, trial)) return r;
        if (int r = project(h, trial, nb, 0, 1000, 1e-12, proj, nullptr, nullptr)) return r;
        if (int r = launch(h, qt::k_fwd64_nll, dim3(nb * nt), dim3(256), qt::Fwd64::kLdsBytes, dc, nb, M, vs, vp, x, proj, 1, fpart))
          return r;
        const qt::Mhmc64Step s{j, post ? 1 : 0, keep ? 1 : 0, kept};
        if (int r = launch(h, qt::k_mhmc64_decide_hits, dim3(nb), dim3(K::NT), 0, nb, nt, s, seed, gc0, fpart, proj, x, fcur, cen,
                           thr, a.n_points, dh, da, dd, parked))
          return r;
        if (post) {
          if (keep) {
            if (!hs) {
              if (int r = metric == QT_METRIC_TRACE
                              ? launch(h, qt::k_metric_dist_dim64<qt::kMetricTrace>, dim3(nb), dim3(W::NT), W::kLdsBytes, parked,
                                       nb, cen, nb, 0, h->jtol2, value)
                              : launch(h, qt::k_metric_dist_dim64<qt::kMetricInfidelity>, dim3(nb), dim3(W::NT), W::kLdsBytes,
                                       parked, nb, cen, nb, 0, h->jtol2, value))
                return r;
              if (int r = launch(h, qt::k_mhmc64_tally, dim3((nb + 255) / 256), dim3(256), 0, nb, value, thr, a.n_points, kept, dh,
                                 dd))
                return r;
            }
            ++kept;
            to_keep = a.thinning;
          }
          --to_keep;
        }
      }
    }
    HIPCHK(hipGetLastError());
    return 0;
  };
  return mhmc_hits_call(h, fn, hs, metric, counts, C, centres, choi_init, thresholds, burn_steps, n_points, thinning, hits, accepted,
                        dist, flags, refuse, launch_chains);
}

int qt_mhmc_process_large_hits(qt_handle_t* h, const int64_t* counts, int C, const double* centres, const double* choi_init,
                               const double* thresholds, uint64_t seed, uint64_t first_chain, int burn_steps, int n_points,
                               int thinning, double step, int64_t* hits, int64_t* accepted, double* dist, int flags) {
  return mhmc_process_large_hits_impl(h, "qt_mhmc_process_large_hits", true, 0, counts, C, centres, choi_init, thresholds, seed,
                                      first_chain, burn_steps, n_points, thinning, step, hits, accepted, dist, flags);
}

int qt_mhmc_process_large_metric_hits(qt_handle_t* h, int metric, const int64_t* counts, int C, const double* centres,
                                      const double* choi_init, const double* thresholds, uint64_t seed, uint64_t first_chain,
                                      int burn_steps, int n_points, int thinning, double step, int64_t* hits,
                                      int64_t* accepted, double* dist, int flags) {
  return mhmc_process_large_hits_impl(h, "qt_mhmc_process_large_metric_hits", false, metric, counts, C, centres, choi_init,
                                      thresholds, seed, first_chain, burn_steps, n_points, thinning, step, hits, accepted, dist,
                                      flags);
}

}  // extern "C"

#ifdef QT_PHASE_TIMING
extern "C" int qt_debug_set_diag(int v) {  // which compile-time variant of k_lifp_gemm<16, 2> the next qt_lifp_batch launches
  g_host_diag = v;
  return 0;
}
// profile build only (scripts/phase_timing.py): where the kernels drop their phase stamps
extern "C" int qt_debug_set_prof(void* device_ptr) {
  long long* p = static_cast<long long*>(device_ptr);
  return hipMemcpyToSymbol(HIP_SYMBOL(qt::g_qt_prof), &p, sizeof(p)) == hipSuccess ? 0 : -3;
}
#endif

// (Behind everything else, so that the device code of the kernels above keeps its place in the code object.)
namespace {

// ---- the 'states' process estimator behind qt_states_choi_batch and its siblings (qt_states_choi.h) ------------------
// f(std::integral_constant<int, d>()) for the handle's d = 2, 4, 8 (the callers have refused n > 3)
template <class F>
int by_small_d(const qt_handle_t* h, F f) {
  switch (h->d) {
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
  }
}

// the test of B matrices into dok[B] and, when wanted, the failing flags dfail[B + 1] (k_choi_is_cptp)
int launch_is_cptp(qt_handle_t* h, const double* dchoi, int B, double atol, int32_t* dok, int32_t* dfail) {
  return by_small_d(h, [&](auto dc) {
    using W = qt::StatesChoi<decltype(dc)::value>;
    return launch(h, qt::k_choi_is_cptp<decltype(dc)::value>, dim3((B + W::TPB - 1) / W::TPB), dim3(W::NT), W::kTestLds, dchoi, B,
                  atol, dok, dfail);
  });
}

// The conditional projection of B assembled matrices on the device, in place: the test (is_cptp's atol = 1e-5), the
// failing trials compacted in batch order (an exclusive sum of their flags), the projection launcher of
// qt_cptp_project_batch(mode 0, n_iter 1000, tol 1e-12) on the compacted copy, and its results put back.  The number of
// failing trials comes back to the host -- ONE read-back, for which the stream is waited for -- since it sizes the
// projection's launch and workspaces.  projected[B] / iters[B] (either may be null) are written for every trial.
int project_failing(qt_handle_t* h, double* dchoi, int B, int32_t* dproj, int32_t* dit) {
  const int ne2 = h->D * h->D * 2;
  HIPCHK(h->sc_ok.ensure((size_t)B * sizeof(int32_t)));
  HIPCHK(h->sc_fail.ensure(((size_t)B + 1) * sizeof(int32_t)));
  HIPCHK(h->sc_pos.ensure(((size_t)B + 1) * sizeof(int32_t)));
  int32_t *ok = h->sc_ok.as<int32_t>(), *failing = h->sc_fail.as<int32_t>(), *pos = h->sc_pos.as<int32_t>();
  if (int r = launch_is_cptp(h, dchoi, B, 1e-5, ok, failing)) return r;
  size_t tmp_bytes = 0;
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, failing, pos, B + 1, h->stream));
  HIPCHK(h->sc_tmp.ensure(tmp_bytes));
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(h->sc_tmp.p, tmp_bytes, failing, pos, B + 1, h->stream));
  int32_t n_fail = 0;
  char* m = mail_alloc(h, sizeof(int32_t));
  HIPCHK(hipMemcpyAsync(m ? (void*)m : (void*)&n_fail, pos + B, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (int r = wait_stream(h)) return r;
  if (m) memcpy(&n_fail, m, sizeof(int32_t));
  if (n_fail < 0 || n_fail > B) return fail(QT_ERR_HIP, "states_choi: %d of %d trials reported as failing", n_fail, B);
  if (n_fail > 0) {
    HIPCHK(h->sc_in.ensure((size_t)n_fail * ne2 * sizeof(double)));
    HIPCHK(h->sc_out.ensure((size_t)n_fail * ne2 * sizeof(double)));
    HIPCHK(h->sc_iters.ensure((size_t)n_fail * sizeof(int32_t)));
    const int r = by_small_d(h, [&](auto dc) {
      return launch(h, qt::k_choi_gather<decltype(dc)::value>, dim3(B), dim3(256), 0, (const double*)dchoi, B, (const int32_t*)ok,
                    (const int32_t*)pos, h->sc_in.as<double>());
    });
    if (r) return r;
    if (int r = project(h, h->sc_in.as<double>(), n_fail, 0, 1000, 1e-12, h->sc_out.as<double>(), h->sc_iters.as<int32_t>(), nullptr))
      return r;
  }
  if (n_fail > 0 || dproj || dit)
    return by_small_d(h, [&](auto dc) {
      return launch(h, qt::k_choi_scatter<decltype(dc)::value>, dim3(B), dim3(256), 0, h->sc_out.as<const double>(),
                    h->sc_iters.as<const int32_t>(), B, (const int32_t*)ok, (const int32_t*)pos, dchoi, dproj, dit);
    });
  return 0;
}

// qt_states_choi_batch (`with_dist` false) and qt_states_choi_dist_group_batch.  The batch runs in slices of 128 MB of Choi
// matrices (524 288 trials at n = 1, 32 768 at n = 2, 2048 at n = 3), so that every workspace that follows the batch stays
// bounded; with cptp there is one read-back (project_failing) per slice.  The same bits whatever the slice: every kernel
// here treats a trial by itself.
int states_choi_impl(qt_handle_t* h, bool with_dist, const double* states, int B, const double* weights, int cptp,
                     const double* centres, int G, double* choi, double* dist, int32_t* projected, int32_t* iters, int flags,
                     const char* fn) {
  QT_ENTER(h);
  Call c(h, flags, fn);
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "%s: process tomography supports n_qubits 1..3 in this release", fn);
  if (int r = need_povm(h)) return r;
  if (!h->proc_set) return fail(QT_ERR_STATE, "qt_process_setup has not been called");
  if (B < 0 || G < 1 || (B > 0 && (!states || !weights || (with_dist ? !centres || !dist : !choi))))
    return fail(QT_ERR_ARG, "bad %s arguments", fn + 3);
  if (B == 0) return 0;
  const int D = h->D;
  const size_t ne2 = (size_t)D * D * 2;
  const double *ds, *dw, *dcen;
  double *dchoi, *ddist;
  int32_t *dproj, *dit;
  if (int r = c.in(states, (size_t)B * ne2, &ds)) return r;
  if (int r = c.in(weights, ne2, &dw)) return r;
  if (int r = c.in(centres, with_dist ? (size_t)G * ne2 : 0, &dcen)) return r;
  if (int r = c.out(choi, (size_t)B * ne2, &dchoi)) return r;
  if (int r = c.out(with_dist ? dist : nullptr, (size_t)B, &ddist)) return r;
  if (int r = c.out(projected, (size_t)B, &dproj)) return r;
  if (int r = c.out(iters, (size_t)B, &dit)) return r;
  const int slice = (int)(((size_t)128 << 20) / (ne2 * sizeof(double)));
  for (int b0 = 0; b0 < B; b0 += slice) {
    const int nb = B - b0 < slice ? B - b0 : slice;
    double* m = dchoi ? dchoi + (size_t)b0 * ne2 : nullptr;
    if (!m) {
      HIPCHK(h->sc_choi.ensure((size_t)nb * ne2 * sizeof(double)));
      m = h->sc_choi.as<double>();
    }
    const int r = by_small_d(h, [&](auto dc) {
      using W = qt::StatesChoi<decltype(dc)::value>;
      return launch(h, qt::k_states_choi<decltype(dc)::value>, dim3((nb + W::TPB - 1) / W::TPB), dim3(W::NT), W::kAssemblyLds,
                    ds + (size_t)b0 * ne2, nb, dw, m);
    });
    if (r) return r;
    if (cptp) {
      if (int r2 = project_failing(h, m, nb, dproj ? dproj + b0 : nullptr, dit ? dit + b0 : nullptr)) return r2;
    }
    if (ddist)
      if (int r2 = launch(h, qt::k_hs_dist, dim3(nb), dim3(64), 0, D, (const double*)m, dcen, G, b0 % G, nb, ddist + b0)) return r2;
  }
  if (!cptp) {
    if (dproj) HIPCHK(hipMemsetAsync(dproj, 0, (size_t)B * sizeof(int32_t), h->stream));
    if (dit) HIPCHK(hipMemsetAsync(dit, 0, (size_t)B * sizeof(int32_t), h->stream));
  }
  return c.done();
}

}  // namespace

extern "C" {

int qt_states_choi_batch(qt_handle_t* h, const double* states, int B, const double* weights, int cptp, double* choi,
                         int32_t* projected, int32_t* iters, int flags) {
  return states_choi_impl(h, false, states, B, weights, cptp, nullptr, 1, choi, nullptr, projected, iters, flags, __func__);
}

int qt_states_choi_dist_group_batch(qt_handle_t* h, const double* states, int B, const double* weights, int cptp,
                                    const double* centres, int G, double* choi, double* dist, int32_t* projected, int32_t* iters,
                                    int flags) {
  return states_choi_impl(h, true, states, B, weights, cptp, centres, G, choi, dist, projected, iters, flags, __func__);
}

int qt_choi_is_cptp_batch(qt_handle_t* h, const double* choi, int B, double atol, int32_t* ok, int flags) {
  QT_ENTER(h);
  Call c(h, flags);
  if (h->nq > 3) return fail(QT_ERR_UNSUPPORTED, "qt_choi_is_cptp_batch: process tomography supports n_qubits 1..3 in this release");
  if (B < 0 || !(atol >= 0.0) || !std::isfinite(atol) || (B > 0 && (!choi || !ok))) return fail(QT_ERR_ARG, "bad choi_is_cptp_batch arguments");
  if (B == 0) return 0;
  const double* dchoi;
  int32_t* dok;
  if (int r = c.in(choi, (size_t)B * h->D * h->D * 2, &dchoi)) return r;
  if (int r = c.out(ok, (size_t)B, &dok)) return r;
  if (int r = launch_is_cptp(h, dchoi, B, atol, dok, nullptr)) return r;
  return c.done();
}

}  // extern "C"
