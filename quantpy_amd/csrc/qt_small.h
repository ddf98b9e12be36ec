// Wave-synchronous kernels for n <= 3 qubits (D = 4^n <= 64 = one wavefront).
//
// Mapping: one trial is owned by a group of G = D lanes of a 64-wide wavefront (64/G trials per
// wave; at n = 3 one trial per wave).  Lane l of a group plays three roles at once:
//   - Bloch / parameter index k = l  (vectors b, w, x, g of length D live one element per lane),
//   - matrix element (i, j) = (l / d, l % d) of every d x d complex matrix (rho, L, G, V),
//   - row m = c*G + l of the M-row POVM contraction, chunk by chunk.
// A workgroup is WPB = 4 waves, one per SIMD of a CU; the waves run independently (wave-level
// fences only), so trials diverge freely inside BFGS.  A dense (M x D) operand -- the left inverse
// for 'lin', the weighted POVM A' for the NLL -- is streamed from L2 by every wave (dot_global:
// 16 loads in flight per lane); a product POVM needs no dense operand at all (ProductView).  An
// LDS-resident operand image shared by the waves was measured slower in both regimes and removed
// (profiles/round1_v3_*).  Per-trial scratch (rho, L, V, b, r, f: ~7 KB) lives in LDS behind the
// workgroup's product-POVM tables; the BFGS inverse Hessian (D x D f64) lives in registers, one
// row per lane (n = 1, 2; n = 3 runs the two-loop form).
//
// Reference semantics implemented (paths into /root/reference/quantpy):
//   lin:  tomography/state.py:191-202, PSD clip :267-273
//   chol: routines.py:84-101
//   nll:  tomography/state.py:217-229 (value); gradient derived analytically
//   mle:  tomography/state.py:204-215 with scipy's BFGS control flow (qt_linesearch.h)
//
// Here: Small<NQ> and the estimator kernels that are thin wrappers over it.  Around it: the wave-level primitives in
// qt_wave.h, the POVM views and per-trial argument structs in qt_args.h, the MLE drivers in qt_mle_small.h, the
// Metropolis-Hastings chains in qt_mhmc_state.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_args.h"
#include "qt_wave.h"

namespace qt {

constexpr bool kLiftSingleNegative = true;  // a7 short cut of Small::lift_single_negative (n = 3)

// Two parts of the n = 3 specialised MLE kernels that can be built without (-DNAME=0), for the A/B libraries of
// profiles/lane_constants_headline_ab.txt.
#ifndef QT_LANE_INT_FRONT
#define QT_LANE_INT_FRONT 1    // load_freq sums counts below 2^22 as 32-bit integers
#endif
#ifndef QT_LANE_LEFTOVERS
#define QT_LANE_LEFTOVERS 1    // no second store of the Bloch element in nll_grad; ballots for the first gradient norm
#endif
constexpr bool kLaneLeftovers = QT_LANE_LEFTOVERS != 0;
// Two re-orderings of the clipped trial's chain in k_mle_fused_hw<3, .> that move no floating-point operation, each
// built without by -DNAME=0 (profiles/lift_tail_headline_ab.txt; three more were measured there and are not in the source):
#ifndef QT_LIFT_ONE_EXIT
#define QT_LIFT_ONE_EXIT 1     // lift_single_negative: the result beside the residual check, one test behind both
#endif
#ifndef QT_EARLY_OUTPUTS
#define QT_EARLY_OUTPUTS 1     // mle_fused_body: the start matrix and the common scalars are stored in front of the evaluation
#endif
constexpr bool kLiftOneExit = QT_LIFT_ONE_EXIT != 0;
constexpr bool kEarlyOutputs = QT_EARLY_OUTPUTS != 0;

template <int NQ>
struct Small {
  static constexpr int d = 1 << NQ;
  static constexpr int D = d * d;
  static constexpr int G = D;
  static constexpr int TPW = 64 / G;       // trials per wave
  static constexpr int WPB = 4;            // waves per workgroup
  static constexpr int NT = 64 * WPB;      // threads per workgroup
  static constexpr int TPB = TPW * WPB;    // trials per workgroup
  static constexpr int T = d * (d - 1) / 2;
  // Row pitch of the d x d complex matrix images: 9 at d = 8, so that the rows one column is read
  // from (pitch 144 B = 36 banks) fall on distinct LDS banks; a pitch of 8 (128 B) makes every such
  // ds_read_b128 a 4-way bank conflict.  d = 2, 4 have no conflict to begin with.
  static constexpr int LD = d == 8 ? 9 : d;
  static constexpr int MAT = 2 * LD * d;   // doubles per matrix image
  // per-trial LDS scratch, in doubles
  static constexpr int oA = 0;             // complex [d][LD]
  static constexpr int oB = oA + MAT;      // complex [d][LD]
  static constexpr int oVec = oB + MAT;    // [D] + one slot that always holds 0 (source of L's zero entries)
  static constexpr int oLam = oVec + D + 2;  // [d] (+ pad to even)
  static constexpr int oM = oLam + 2 * ((d + 1) / 2);  // rbuf[Mp], freq[Mp], bufB[Mp]
  // The third matrix image V (eigenvectors / projector / speculative inverse: make_feasible only) lives on top of rbuf
  // whenever rbuf is large enough: rbuf is a staging buffer of load_freq, lin_invert and nll_grad, none of which is
  // in flight while make_feasible runs.  At n = 3 with the 216-row POVM that takes a trial from 9.2 to 8.1 KB and a
  // 4-trial workgroup from 42.9 to 38.3 KB of LDS: FOUR workgroups per CU instead of three (the saturated batches
  // were LDS-limited to 3 waves per SIMD with registers for 4).
  __host__ __device__ static bool v_on_rbuf(int M) { return ((M + 1) & ~1) >= MAT; }
  __host__ __device__ static int v_offset(int M, int R1) {
    const int Mp = (M + 1) & ~1;
    return v_on_rbuf(M) ? oM : oM + (R1 > 0 ? 3 : 2) * Mp;
  }
  __host__ __device__ static int trial_doubles(int M, int R1 = 0) {
    const int Mp = (M + 1) & ~1;
    return oM + (R1 > 0 ? 3 : 2) * Mp + (v_on_rbuf(M) ? 0 : MAT);
  }
  // Index tables of a product POVM, staged once per workgroup (shared by its waves): forward stage
  // tables, backward stage tables, R-order row map.
  __host__ __device__ static int ipow_h(int b, int e) {
    int r = 1;
    for (int t = 0; t < e; ++t) r *= b;
    return r;
  }
  __host__ __device__ static int fwd_ints(int R1) {
    int t = 0;
    for (int q = 1; q <= NQ; ++q) t += ipow_h(R1, q) << (2 * (NQ - q));
    return t;
  }
  __host__ __device__ static int bwd_ints(int R1) {
    int t = 0;
    for (int q = 1; q <= NQ; ++q) t += ipow_h(R1, q - 1) << (2 * (NQ - q + 1));
    return t;
  }
  __host__ __device__ static int table_ints(int M, int R1) { return (fwd_ints(R1) + bwd_ints(R1) + M + 1) & ~1; }
  __host__ __device__ static int table_doubles(int M, int R1) {
    // index tables, then the row weights wrowR[M] (padded to even), then the one-qubit tables T and pinv(T)^T
    // ([R1][4] each, 16-byte aligned): staged ONCE per workgroup.  (The one-qubit tables used to be copied per trial
    // inside load_freq: two dependent global loads on the critical path of a lone wave, ~1 us of the 16 us step.)
    return R1 > 0 ? (table_ints(M, R1) / 2 + ((M + 1) & ~1) + 8 * R1) : 0;
  }
  __host__ __device__ static size_t lds_bytes(int M, int R1 = 0, int extra = 0) {
    return ((size_t)table_doubles(M, R1) + (size_t)TPB * (trial_doubles(M, R1) + extra)) * sizeof(double);
  }
  // k_mle_fused_hw: behind that, one more scratch (without `extra`) per trial, for its twin wavefront
  __host__ __device__ static int twin_offset(int M, int R1, int extra) {
    return table_doubles(M, R1) + TPB * (trial_doubles(M, R1) + extra);
  }
  __host__ __device__ static size_t lds_bytes_twin(int M, int R1, int extra) {
    return lds_bytes(M, R1, extra) + (size_t)TPB * trial_doubles(M, R1) * sizeof(double);
  }

  // ---- per-lane context ---------------------------------------------------------------
  struct Ctx {
    int l, i, j, e;  // lane in group, matrix element, its slot i * LD + j in a matrix image
    double* sm;      // this trial's LDS scratch
    const int *tfwd, *tbwd, *trmap;  // the workgroup's copy of the product-POVM index tables (LDS)
    const double* twrow;             // ... and of the row weights N_s / sum(N), R-order
    const double *ttab, *ptab;       // ... and of the one-qubit tables T [R1][4], pinv(T)^T [R1][4]
    int M, Mp;
    PovmView pv;
    // Pauli string k = l:  P_k[r][r ^ xm] = (-i)^ny (-1)^popc(r & zm)
    int xm, zm, ny;
    // Cholesky parameter owned by lane l: element (pi, pj), kind 0 diag / 1 real / 2 imag
    int pi, pj, pkind;
    // where element (i, j) of L finds its real / imaginary part in the parameter vector (D = the zero slot)
    int src_re, src_im;
    __device__ __forceinline__ cd* A() const { return reinterpret_cast<cd*>(sm + oA); }
    __device__ __forceinline__ cd* Bm() const { return reinterpret_cast<cd*>(sm + oB); }
    __device__ __forceinline__ cd* V() const { return reinterpret_cast<cd*>(sm + v_offset(M, pv.pr.enabled ? pv.pr.R1 : 0)); }
    __device__ __forceinline__ double* vec() const { return sm + oVec; }
    __device__ __forceinline__ double* lam() const { return sm + oLam; }
    __device__ __forceinline__ double* rbuf() const { return sm + oM; }
    __device__ __forceinline__ double* freq() const { return sm + oM + Mp; }
    __device__ __forceinline__ double* bufB() const { return sm + oM + 2 * Mp; }
    __device__ __forceinline__ const double* tabT() const { return ttab; }  // [R1][4]
    __device__ __forceinline__ const double* tabP() const { return ptab; }  // [R1][4]
    __device__ __forceinline__ bool prod() const { return pv.pr.enabled != 0; }
    __device__ __forceinline__ double* extra() const { return sm + trial_doubles(M, pv.pr.enabled ? pv.pr.R1 : 0); }  // [pv.extra]
    // the launch-uniform facts, read at run time here and compile-time constants in CtxS
    static constexpr bool kGeneric = true;
    static constexpr int kLaneTables = 0;   // (CtxSV)
    static constexpr bool kHelper = false;  // (WithHelper)
    // (CtxH: the helper wavefront's lift can be called off; a trial's own never is)
    __device__ __forceinline__ static constexpr int verdict_load() { return 0; }
    __device__ __forceinline__ static constexpr bool abandoned(int) { return false; }
    __device__ __forceinline__ int R1() const { return pv.pr.R1; }
    __device__ __forceinline__ bool uniform() const { return pv.pr.uniform != 0; }
    __device__ __forceinline__ bool pairedT() const { return pv.pr.pairedT != 0; }
    __device__ __forceinline__ bool pairedP() const { return pv.pr.pairedP != 0; }
    __device__ __forceinline__ double wuni() const { return pv.pr.wuni; }
    __device__ __forceinline__ double jtol2() const { return pv.jtol2; }
    __device__ __forceinline__ double cT(int k) const { return pv.pr.cT[k]; }
    __device__ __forceinline__ double cP(int k) const { return pv.pr.cP[k]; }
  };
  // The context of the specialised kernels (SpecArgs): the same roles, the shape known to the compiler.  The table
  // block holds the image of SpecArgs::image and nothing else; the trial scratch keeps the generic layout and offset.
  // LT: where the lane tables of matrix_of / bloch_of at n = 3 live.  2: decoded in vector registers -- the kernels that
  // run one wavefront per SIMD with registers to spare (k_mle_fused*).  1: two packed words per lane, decoded at each
  // call (k_mle_start, held to 128 VGPRs).  0: no lane tables, the forms of the generic context (k_mle_bfgs: with the
  // tables its allocation ended at 181 registers instead of 165, above the 168 of three waves per SIMD, and the
  // saturated iterating batches ran 10-20 % slower, profiles/mle_diet_headline_ab.txt).
  template <int LT>
  struct CtxSV {
    static constexpr bool VC = LT == 2;
    int l, i, j, e;
    double* sm;
    const int* tfwd;            // `last`: the stage-n entries
    const double *ttab, *ptab;  // T [6][4], pinv(T)^T [6][4]
    int M, Mp;
    SpecArgs a;
    int xm, zm, ny;
    int pi, pj, pkind;
    int src_re, src_im;
    int bslot;  // n = 3: where bloch_of's lane (x, z) leaves its value, pauli_index(x, z)
    // The 12 + 12 coefficients of the paired stages.  k_mle_start / k_mle_bfgs (held to 128 / 168 VGPRs) keep them as
    // scalars: without the PovmView they fit the SGPR file.  k_mle_fused does not get them to fit -- its BFGS loop and
    // the f64 literals of fast_log are scalars too, and the register allocator's answer was to spill all 24 at the top
    // of nll_grad and restore them lane by lane in front of every stage (158 v_readlane per evaluation) -- but it runs
    // one wave per SIMD with ~75 VGPRs to spare: there they are pinned in vector registers (make_ctx<true>), where an
    // FMA reads them at no cost.
    double kT[12], kP[12];
    // matrix_of (n = 3): the d terms of this lane in the order they are added (mat_slots), a byte each: Bloch index k,
    // bit 7 = negative.  VC: decoded once into the term's address in vec() and the mask that flips its sign.
    uint32_t mpack[2];
    const double* mterm[VC ? d : 1];
    uint32_t msign[VC ? d : 1];
    // bloch_of (n = 3), VC: the sign masks of the butterfly's three stages (lane & 1, 2, 4) and of the phase
    uint32_t bflip[VC ? 4 : 1];
    static constexpr int kLaneTables = LT;
    __device__ __forceinline__ cd* A() const { return reinterpret_cast<cd*>(sm + oA); }
    __device__ __forceinline__ cd* Bm() const { return reinterpret_cast<cd*>(sm + oB); }
    __device__ __forceinline__ cd* V() const { return reinterpret_cast<cd*>(sm + v_offset(M, 6)); }
    __device__ __forceinline__ double* vec() const { return sm + oVec; }
    __device__ __forceinline__ double* lam() const { return sm + oLam; }
    __device__ __forceinline__ double* rbuf() const { return sm + oM; }
    __device__ __forceinline__ double* freq() const { return sm + oM + Mp; }
    __device__ __forceinline__ double* bufB() const { return sm + oM + 2 * Mp; }
    __device__ __forceinline__ const double* tabT() const { return ttab; }
    __device__ __forceinline__ const double* tabP() const { return ptab; }
    __device__ __forceinline__ double* extra() const { return sm + trial_doubles(M, 6); }  // [a.extra]
    static constexpr bool kGeneric = false;
    static constexpr bool kHelper = false;
    __device__ __forceinline__ static constexpr int verdict_load() { return 0; }
    __device__ __forceinline__ static constexpr bool abandoned(int) { return false; }
    __device__ __forceinline__ static constexpr bool prod() { return true; }
    __device__ __forceinline__ static constexpr int R1() { return 6; }
    __device__ __forceinline__ static constexpr bool uniform() { return true; }
    __device__ __forceinline__ static constexpr bool pairedT() { return true; }
    __device__ __forceinline__ static constexpr bool pairedP() { return true; }
    __device__ __forceinline__ double wuni() const { return a.wuni; }
    __device__ __forceinline__ double jtol2() const { return a.jtol2; }
    __device__ __forceinline__ double cT(int k) const { return kT[k]; }
    __device__ __forceinline__ double cP(int k) const { return kP[k]; }
  };
  using CtxS = CtxSV<1>;
  __device__ __forceinline__ static double pin_vgpr(double x) {  // the value, in a vector register from here on
    asm volatile("" : "+v"(x));
    return x;
  }
  template <bool GENERIC, class = void>
  struct CtxOf {
    using type = Ctx;
  };
  template <class X>
  struct CtxOf<false, X> {
    using type = CtxSV<1>;
  };
  // 16-byte chunks of the table image (SpecArgs::image): `last` padded to four entries, then the two one-qubit tables
  __host__ __device__ static int image_last_ints(int M) { return (M + 3) & ~3; }
  // (M = 6^n <= 216: at most 78 chunks, one per thread of the workgroup)
  __host__ __device__ static int image_chunks(int M) { return image_last_ints(M) / 4 + 2 * 24 / 2; }

  // Trial handled by this lane's group; *live = false for the padding groups of the last block.
  __device__ __forceinline__ static int trial_index(int B, bool* live) {
    const int wave = threadIdx.x >> 6, tib = (threadIdx.x & 63) / G;
    const int b = (blockIdx.x * WPB + wave) * TPW + tib;
    *live = b < B;
    return b;
  }

  // TWIN (k_mle_fused_hw): the workgroup has a second wavefront per trial (`twin` != 0, wave-uniform), which comes
  // through here like the first, leaves the staging of the tables to it, and gets a scratch of its own (twin_offset).
  template <bool TWIN = false>
  __device__ static void make_ctx(Ctx& c, double* smem_block, const PovmView& pv, [[maybe_unused]] int twin = 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c.l = lane % G;
    const int slot = wave * TPW + lane / G;
    c.i = c.l / d;
    c.j = c.l % d;
    c.e = c.i * LD + c.j;
    c.M = pv.M;
    c.Mp = (pv.M + 1) & ~1;
    c.pv = pv;
    const int r1 = pv.pr.enabled ? pv.pr.R1 : 0;
    int* tabs = reinterpret_cast<int*>(smem_block);
    c.tfwd = tabs;
    c.tbwd = tabs + fwd_ints(r1);
    c.trmap = c.tbwd + bwd_ints(r1);
    double* wrow = smem_block + table_ints(pv.M, r1) / 2;
    double* t1 = wrow + ((pv.M + 1) & ~1);
    c.twrow = wrow;
    c.ttab = t1;
    c.ptab = t1 + 4 * r1;
    if (r1 > 0) {  // every thread of the workgroup comes through here once, before anything else
      const int nf = fwd_ints(r1), nb = bwd_ints(r1);
      if (!(TWIN && twin)) {
        for (int e = threadIdx.x; e < 4 * r1; e += NT) {
          t1[e] = pv.pr.T[e];
          t1[4 * r1 + e] = pv.pr.P1T[e];
        }
        // paired tables index their stages in closed form: only stage n of the forward pass keeps a table (M <= nf
        // entries, in the place of the forward tables)
        if (pv.pr.pairedT) {
          for (int e = threadIdx.x; e < pv.M; e += NT) tabs[e] = pv.pr.last[e];
        } else {
          for (int e = threadIdx.x; e < nf; e += NT) tabs[e] = pv.pr.fwd[e];
        }
        if (!(pv.pr.pairedT && pv.pr.pairedP))
          for (int e = threadIdx.x; e < nb; e += NT) tabs[nf + e] = pv.pr.bwd[e];
        for (int e = threadIdx.x; e < pv.M; e += NT) {
          tabs[nf + nb + e] = pv.pr.rmap[e];
          wrow[e] = pv.pr.wrowR[e];
        }
      }
      __syncthreads();
    }
    c.sm = smem_block + table_doubles(pv.M, r1) + slot * (trial_doubles(pv.M, r1) + pv.extra);
    if (TWIN && twin) c.sm = smem_block + twin_offset(pv.M, r1, pv.extra) + slot * trial_doubles(pv.M, r1);
    int xm = 0, zm = 0, ny = 0;
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
      const int dig = (c.l >> (2 * b)) & 3;
      if (dig == 1 || dig == 2) xm |= 1 << b;
      if (dig == 2 || dig == 3) zm |= 1 << b;
      if (dig == 2) ++ny;
    }
    c.xm = xm;
    c.zm = zm;
    c.ny = ny & 3;
    if (c.l < d) {
      c.pi = c.pj = c.l;
      c.pkind = 0;
    } else {
      int t = c.l - d;
      c.pkind = 1;
      if (t >= T) {
        t -= T;
        c.pkind = 2;
      }
      int ii = 1;
      while ((ii * (ii + 1)) / 2 <= t) ++ii;  // row of np.tril_indices(d, -1)[t]
      c.pi = ii;
      c.pj = t - (ii * (ii - 1)) / 2;
    }
    c.src_re = c.src_im = D;
    if (c.i == c.j) c.src_re = c.i;
    else if (c.i > c.j) {
      const int tt = (c.i * (c.i - 1)) / 2 + c.j;
      c.src_re = d + tt;
      c.src_im = d + T + tt;
    }
    if (c.l == 0) c.sm[oVec + D] = 0.0;  // (this trial's scratch: c.sm is set above)
  }

  // Bloch index of the Pauli string with X-type mask x and Z-type mask z.
  __device__ __forceinline__ static int pauli_index(int x, int z) {
    int k = 0;
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
      const int xb = (x >> b) & 1, zb = (z >> b) & 1;
      const int dig = xb ? (zb ? 2 : 1) : (zb ? 3 : 0);
      k |= dig << (2 * b);
    }
    return k;
  }
  // Re[(-i)^ny * s]
  __device__ __forceinline__ static double re_phase(int ny, cd s) {
    return ny == 0 ? s.re : ny == 1 ? s.im : ny == 2 ? -s.re : -s.im;
  }
  // (-i)^ny * v for real v
  __device__ __forceinline__ static cd phase_times(int ny, double v) {
    return ny == 0 ? cd{v, 0.0} : ny == 1 ? cd{0.0, -v} : ny == 2 ? cd{-v, 0.0} : cd{0.0, v};
  }

  // b_k = Re Tr(P_k M^dagger) / d for the matrix held in LDS `m` (qobj.py:132).
  // n = 3 (one trial per wavefront, lane = 8 x + r): as in qt_large.h, for a fixed x-mask the eight strings (x, z) make
  // the sum over r a length-8 Walsh-Hadamard transform of the shifted diagonal M[r][r ^ x] -- one LDS read and three
  // butterfly stages across the lanes (two quad_perm DPP moves, one ds_bpermute) instead of eight reads and eight
  // sign-and-accumulate steps per lane (~85 -> ~40 vector instructions); the value lands in lane (x, z) and goes to
  // lane k = pauli_index(x, z) through c.vec(), which the caller fills with the Bloch vector anyway.
  __device__ __forceinline__ static cd wht_step(cd s, cd p, bool upper) {
    return upper ? cd{p.re - s.re, p.im - s.im} : cd{s.re + p.re, s.im + p.im};
  }
  template <class C>
  __device__ static double bloch_of(const C& c, const cd* m) {
    if constexpr (NQ == 3) {
      const int x = c.i, r = c.j, lane = threadIdx.x & 63;
      const cd e = m[r * LD + (r ^ x)];
      cd s{e.re, -e.im};
      if constexpr (C::kLaneTables != 0) {
        // the same sums without a select: p - s is p + (-s), and whether a lane subtracts is a lane constant -- a sign
        // mask per stage, held in registers (CtxSV<2>) or formed from the lane number (CtxSV<1>)
        uint32_t f[4];
        if constexpr (C::kLaneTables == 2) {
#pragma unroll
          for (int b = 0; b < 4; ++b) f[b] = c.bflip[b];
        } else {
          f[0] = (uint32_t)lane << 31;
          f[1] = ((uint32_t)lane << 30) & 0x80000000u;
          f[2] = ((uint32_t)lane << 29) & 0x80000000u;
          f[3] = ((uint32_t)__popc(x & r) << 30) & 0x80000000u;
        }
        s = cd{flip_sign(s.re, f[0]) + dpp_f64<0xB1>(s.re), flip_sign(s.im, f[0]) + dpp_f64<0xB1>(s.im)};
        s = cd{flip_sign(s.re, f[1]) + dpp_f64<0x4E>(s.re), flip_sign(s.im, f[1]) + dpp_f64<0x4E>(s.im)};
        s = cd{flip_sign(s.re, f[2]) + __shfl_xor(s.re, 4), flip_sign(s.im, f[2]) + __shfl_xor(s.im, 4)};
        // Re[(-i)^ny s], ny = popc(x & z): s.re, s.im, -s.re, -s.im
        const double v = flip_sign((__popc(x & r) & 1) ? s.im : s.re, f[3]) / d;
        double* vec = c.vec();
        vec[c.bslot] = v;
        wave_sync();
        const double mine = vec[c.l];
        wave_sync();
        return mine;
      }
      s = wht_step(s, cd{dpp_f64<0xB1>(s.re), dpp_f64<0xB1>(s.im)}, lane & 1);
      s = wht_step(s, cd{dpp_f64<0x4E>(s.re), dpp_f64<0x4E>(s.im)}, lane & 2);
      s = wht_step(s, cd{__shfl_xor(s.re, 4), __shfl_xor(s.im, 4)}, lane & 4);
      const int z = r;
      const double v = re_phase(__popc(x & z) & 3, s) / d;
      // pauli_index(x, z): digit bits (hi, lo) = (z_q, x_q ^ z_q) = spread(x) ^ 3 spread(z)
      const int sx = (x & 1) | ((x & 2) << 1) | ((x & 4) << 2), sz = (z & 1) | ((z & 2) << 1) | ((z & 4) << 2);
      double* vec = c.vec();
      if constexpr (C::kGeneric) vec[sx ^ (3 * sz)] = v;
      else vec[c.bslot] = v;  // the same index, a lane constant computed once (make_ctx)
      wave_sync();
      const double mine = vec[c.l];
      wave_sync();
      return mine;
    }
    cd s{0.0, 0.0};
#pragma unroll
    for (int r = 0; r < d; ++r) {
      const cd e = m[r * LD + (r ^ c.xm)];  // conj(M[r][r^x]) summed with the sign of P_k[r][r^x]
      const double sg = (__popc(r & c.zm) & 1) ? -1.0 : 1.0;
      s.re += sg * e.re;
      s.im -= sg * e.im;
    }
    return re_phase(c.ny, s) / d;
  }

  // Element (i, j) of sum_k v[k] P_k, v in LDS (qobj.py:114-117).
  // Element (i, j) of sum_k v[k] P_k needs d of the D terms: k = pauli_index(i ^ j, z), z < d, each
  // with phase (-i)^popc(x & z) (-1)^popc(i & z).  Which k, real or imaginary, which sign: one byte
  // per z (k | imaginary << 6 | negative << 7), a pure function of the lane, folded at compile time
  // into a 64-entry table -- the run-time version spent ~25 integer instructions per term on it.
  static constexpr uint64_t mat_pack(int l) {
    const int i = l / d, j = l % d, x = i ^ j;
    uint64_t pack = 0;
    for (int z = 0; z < d; ++z) {
      int k = 0, ny = 0, par = 0;
      for (int b = 0; b < NQ; ++b) {
        const int xb = (x >> b) & 1, zb = (z >> b) & 1;
        const int dig = xb ? (zb ? 2 : 1) : (zb ? 3 : 0);
        k |= dig << (2 * b);
        ny += xb & zb;
        par ^= ((i >> b) & 1) & zb;
      }
      ny &= 3;
      const int imag = ny & 1;                       // (-i)^ny: 1, -i, -1, i
      const int neg = ((ny == 1 || ny == 2) ? 1 : 0) ^ par;
      pack |= (uint64_t)(k | (imag << 6) | (neg << 7)) << (8 * z);
    }
    return pack;
  }
  // The same bytes in the order a lane adds them, without the real / imaginary flag: an off-diagonal element has d / 2
  // real terms and d / 2 imaginary ones (x = i ^ j != 0: popc(x & z) is odd for half of the z), so its real terms in
  // the order of z fill slots 0 .. d/2 - 1 and its imaginary terms the rest; a diagonal element has d real terms and
  // they fill the slots in the order of z.
  static constexpr uint64_t mat_slots(int l) {
    const uint64_t pack = mat_pack(l);
    uint64_t out = 0;
    int n = 0;
    for (int imag = 0; imag < 2; ++imag)
      for (int z = 0; z < d; ++z) {
        const uint64_t e = (pack >> (8 * z)) & 0xffu;
        if ((int)((e >> 6) & 1u) == imag) out |= (e & 0xbfu) << (8 * n++);
      }
    return out;
  }
  template <bool SLOTS, int... L>
  struct MatTab {
    static constexpr uint64_t v[sizeof...(L)] = {(SLOTS ? mat_slots(L) : mat_pack(L))...};
  };
  template <bool SLOTS, int N, int... L>
  struct MakeMatTab : MakeMatTab<SLOTS, N - 1, N - 1, L...> {};
  template <bool SLOTS, int... L>
  struct MakeMatTab<SLOTS, 0, L...> {
    using type = MatTab<SLOTS, L...>;
  };
  static_assert(NQ <= 3, "the packed table holds d <= 8 terms of 8 bits");
  __device__ __forceinline__ static double flip_sign(double v, uint32_t mask) {  // mask 0 / 0x80000000: v / -v, to the bit
    return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) ^ ((uint64_t)mask << 32));
  }
  template <class C>
  __device__ static cd matrix_of(const C& c, const double* v) {
    if constexpr (NQ == 3 && C::kLaneTables != 0) {
      // The specialised start and one-launch kernels: no decision per term is left.  Address and sign of a term are lane
      // constants (CtxSV: decoded in registers, or two packed words), the real and the imaginary sum are one chain of
      // adds over the slots -- for a diagonal element the second half goes on from the first, for the others it starts
      // at zero -- and each lane adds its terms in the order of z as before.  (v is c.vec(): the addresses are decoded
      // for it.)
      double t[d];
#pragma unroll
      for (int s = 0; s < d; ++s) {
        if constexpr (C::kLaneTables == 2) {
          t[s] = flip_sign(*c.mterm[s], c.msign[s]);
        } else {
          const uint32_t w = c.mpack[s / 4];
          const int sh = 8 * (s % 4);
          t[s] = flip_sign(v[(w >> sh) & 63u], (w << (24 - sh)) & 0x80000000u);
        }
      }
      double a = 0.0;
#pragma unroll
      for (int s = 0; s < d / 2; ++s) a += t[s];
      const bool diag = c.i == c.j;
      double b = diag ? a : 0.0;
#pragma unroll
      for (int s = d / 2; s < d; ++s) b += t[s];
      return cd{diag ? b : a, diag ? 0.0 : b};
    }
    using Tab = typename MakeMatTab<false, D>::type;
    const uint64_t pack = Tab::v[c.l];
    cd s{0.0, 0.0};
#pragma unroll
    for (int z = 0; z < d; ++z) {
      const uint32_t e = (uint32_t)(pack >> (8 * z)) & 0xffu;
      double val = v[e & 63u];
      val = (e & 0x80u) ? -val : val;
      if (e & 0x40u) s.im += val;
      else s.re += val;
    }
    return s;
  }

  // counts of this trial -> freq[] in LDS (counts / sum(counts): state.py:193, :227).  For a product
  // POVM the frequencies are stored in R-order and the one-qubit tables are staged next to them.
  // The counts are the only HBM read of a trial.  Issued at the very top of the kernel (before the
  // workgroup stages its tables and meets at the barrier of make_ctx) their latency runs in the shadow
  // of that set-up; up to 4 values per lane are held in registers until load_freq picks them up.
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // (a register value: HIP's uint4 is a struct, copied through memory)
  struct Prefetch {
    int64_t v[4];
    double ns[4];  // N_s of the settings rows l + q G belong to (segmented check) or of setting s = lane (ns[0])
    bool ok, seg;  // seg: K in {2, 4, 8, 16} divides G -- the K outcomes of a setting sit in K neighbouring lanes
    int ri[4];     // specialised kernels: the R-order slots of the rows l + q G (rinv)
    u32x4 img;     // ... and this thread's 16-byte chunk of the workgroup's table image
    uint64_t mat;  // ... and this lane's entry of matrix_of's term table (n = 3: mat_slots)
  };
  __device__ __forceinline__ static void prefetch_counts(Prefetch& pf, const int64_t* counts, const PovmView& pv) {
    const int l = (threadIdx.x & 63) % G, M = pv.M, K = pv.K;
    pf.ok = M <= 4 * G;
    pf.seg = pf.ok && pv.Ns && (K == 2 || K == 4 || K == 8 || K == 16) && G % K == 0;
    const int lgk = __builtin_ctz((unsigned)(K > 0 ? K : 1));  // K is a power of two on the seg path: m / K is a shift
    if (pf.ok) {                                               // (a 32-bit division by a run-time K is ~25 instructions)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = l + q * G;
        pf.v[q] = counts[m < M ? m : M - 1];
        if (pf.seg) pf.ns[q] = pv.Ns[(m < M ? m : M - 1) >> lgk];
      }
    }
    if (!pf.seg) pf.ns[0] = pv.Ns ? pv.Ns[l < pv.S ? l : pv.S - 1] : 0.0;
  }
  // sum over the aligned group of KK neighbouring lanes, KK a compile-time constant (no branch per step)
  template <int KK>
  __device__ __forceinline__ static double segsum_c(double v) {
    v += dpp_f64<0xB1>(v);
    if (KK >= 4) v += dpp_f64<0x4E>(v);
    if (KK >= 8) v += dpp_f64<0x141>(v);
    if (KK >= 16) v += dpp_f64<0x140>(v);
    return v;
  }
  template <int KK>
  __device__ __forceinline__ static bool seg_check(const double (&dv)[4], const bool (&valid)[4], double total,
                                                   const Prefetch& pf, double ns_tot) {
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) bad |= valid[q] & !shots_match(segsum_c<KK>(dv[q]), total, pf.ns[q], ns_tot);
    return bad;
  }
  __device__ static bool load_freq(const Ctx& c, const int64_t* counts, const Prefetch* pf = nullptr) {
    // one coalesced pass over the counts: values parked in rbuf
    double part = 0.0;
    double* raw = c.rbuf();
    double* fq = c.freq();
    bool bad = false;
    double total, inv;
    if (pf && pf->ok) {
      // The prefetched path (M <= 4 G: every built-in POVM at n <= 3) is written WITHOUT branches: out-of-range rows
      // carry 0.0 and go to one dummy slot behind raw[] (the first word of freq[], overwritten below), the frequency
      // pass re-writes row M - 1 from the lanes beyond it, and the shots check is a compile-time butterfly per K.  As
      // `if (m < M)` blocks and a run-time K it compiled to ~25 scalar branches on the critical path of a lone wave.
      double dv[4];
      bool valid[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = c.l + q * G;
        valid[q] = m < c.M;
        dv[q] = valid[q] ? (double)pf->v[q] : 0.0;
        raw[valid[q] ? m : c.Mp] = dv[q];
        part += dv[q];
      }
      total = gsum<G>(part);
      inv = 1.0 / total;
      if (pf->seg) {  // (uniform) the K outcomes of a setting are K neighbouring lanes of one prefetched value
        switch (c.pv.K) {
          case 2: bad = seg_check<2>(dv, valid, total, *pf, c.pv.ns_tot); break;
          case 4: bad = seg_check<4>(dv, valid, total, *pf, c.pv.ns_tot); break;
          case 8: bad = seg_check<8>(dv, valid, total, *pf, c.pv.ns_tot); break;
          default: bad = seg_check<16>(dv, valid, total, *pf, c.pv.ns_tot); break;
        }
      }
      wave_sync();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = c.l + q * G, mc = m < c.M ? m : c.M - 1;
        fq[mc] = raw[c.prod() ? c.trmap[mc] : mc] * inv;
      }
    } else {
      for (int m = c.l; m < c.M; m += G) {
        const double v = (double)counts[m];
        raw[m] = v;
        part += v;
      }
      total = gsum<G>(part);
      inv = 1.0 / total;
      wave_sync();
      if (c.prod()) {
        for (int m = c.l; m < c.M; m += G) fq[m] = raw[c.trmap[m]] * inv;
      } else {
        for (int m = c.l; m < c.M; m += G) fq[m] = raw[m] * inv;
      }
    }
    // shots check (state.py:138-141, 194-197) for the shapes the butterfly does not cover: lane s sums the K outcomes
    // of setting s (raw is in the caller's (S, K) order)
    if (c.pv.Ns && !(pf && pf->seg)) {
      const int K = c.pv.K;
      for (int s = c.l; s < c.pv.S; s += G) {
        double t = 0.0;
        for (int k = 0; k < K; ++k) t += raw[s * K + k];
        const double ns = (pf && s == c.l) ? pf->ns[0] : c.pv.Ns[s];
        bad |= !shots_match(t, total, ns, c.pv.ns_tot);
      }
    }
    const unsigned long long votes = __builtin_amdgcn_ballot_w64(bad);
    const int lane = threadIdx.x & 63;
    const unsigned long long mine = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (lane / G * G));
    wave_sync();
    return (votes & mine) == 0ull;
  }

  // ---- prologue of the specialised kernels (SpecArgs, CtxS) -------------------------------------
  // Everything a trial reads from memory is requested in ONE batch at the top of the kernel: this thread's chunk of
  // the table image (L2), the counts of its rows (the only cold read), their R-order slots and their settings' N_s.
  // make_ctx then has one wait, one ds_write_b128 per thread and the workgroup barrier; the generic body stages its
  // tables in three load -> wait -> write loops, each an exposed L2 round trip of a lone wave.
  __device__ __forceinline__ static void prefetch_counts(Prefetch& pf, const int64_t* counts, const SpecArgs& a) {
    const int l = (threadIdx.x & 63) % G, M = a.M, nch = image_chunks(M), t = threadIdx.x;
    const u32x4* img = reinterpret_cast<const u32x4*>(a.image);
    const int* rinv = reinterpret_cast<const int*>(img + nch);
    pf.img = img[t < nch ? t : nch - 1];
    if constexpr (NQ == 3) pf.mat = MakeMatTab<true, D>::type::v[l];
    pf.ok = pf.seg = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = l + q * G, mc = m < M ? m : M - 1;
      pf.v[q] = counts[mc];
      pf.ri[q] = rinv[mc];
      pf.ns[q] = a.Ns[mc >> NQ];  // K = d outcomes per setting
    }
  }
  // The rest of the argument struct, asked for straight behind the batch above: the 24 coefficients are the second fetch
  // from the argument segment, and requested here their wait falls behind the issue of the counts' loads instead of
  // standing alone in front of the workgroup barrier.  CtxSV::VC: pinned in vector registers, which the one-wave-per-SIMD
  // kernels hold for them through the whole kernel anyway.  make_ctx fills in the rest of the context.
  template <int LT>
  __device__ __forceinline__ static void take_coefs(CtxSV<LT>& c, const SpecArgs& a) {
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      c.kT[k] = CtxSV<LT>::VC ? pin_vgpr(a.cT[k]) : a.cT[k];
      c.kP[k] = CtxSV<LT>::VC ? pin_vgpr(a.cP[k]) : a.cP[k];
    }
  }
  template <bool VCOEF = false, bool TWIN = false, int LT>
  __device__ static void make_ctx(CtxSV<LT>& c, double* smem_block, const SpecArgs& a, const Prefetch& pf,
                                  [[maybe_unused]] int twin = 0) {
    static_assert(VCOEF == (LT == 2), "the one-wave-per-SIMD kernels keep coefficients and lane tables in vector registers");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c.l = lane % G;
    const int slot = wave * TPW + lane / G;
    c.i = c.l / d;
    c.j = c.l % d;
    c.e = c.i * LD + c.j;
    c.M = a.M;
    c.Mp = (a.M + 1) & ~1;
    c.a = a;
    if (!(TWIN && twin) && (int)threadIdx.x < image_chunks(a.M)) reinterpret_cast<u32x4*>(smem_block)[threadIdx.x] = pf.img;
    c.tfwd = reinterpret_cast<const int*>(smem_block);
    c.ttab = smem_block + image_last_ints(a.M) / 2;
    c.ptab = c.ttab + 24;
    c.sm = smem_block + table_doubles(a.M, 6) + slot * (trial_doubles(a.M, 6) + a.extra);
    if (TWIN && twin) c.sm = smem_block + twin_offset(a.M, 6, a.extra) + slot * trial_doubles(a.M, 6);
    if (c.l == 0) c.sm[oVec + D] = 0.0;
    __syncthreads();
    // lane constants, without loops or branches
    int xm = 0, zm = 0, ny = 0;
#pragma unroll
    for (int b = 0; b < NQ; ++b) {
      const int dig = (c.l >> (2 * b)) & 3;
      xm |= (dig == 1 || dig == 2) << b;
      zm |= (dig >= 2) << b;
      ny += dig == 2;
    }
    c.xm = xm;
    c.zm = zm;
    c.ny = ny & 3;
    param_owner(c.l, c.pi, c.pj, c.pkind);
    const int tt = (c.i * (c.i - 1)) / 2 + c.j;
    c.src_re = c.i == c.j ? c.i : c.i > c.j ? d + tt : D;
    c.src_im = c.i > c.j ? d + T + tt : D;
    // bloch_of (n = 3): lane (x, z) = (i, j) holds the value of Pauli string pauli_index(x, z) = spread(x) ^ 3 spread(z)
    const int sx = (c.i & 1) | ((c.i & 2) << 1) | ((c.i & 4) << 2), sz = (c.j & 1) | ((c.j & 2) << 1) | ((c.j & 4) << 2);
    c.bslot = sx ^ (3 * sz);
    if constexpr (NQ == 3 && LT != 0) {
      c.mpack[0] = (uint32_t)pf.mat;
      c.mpack[1] = (uint32_t)(pf.mat >> 32);
      if constexpr (VCOEF) {
#pragma unroll
        for (int s = 0; s < d; ++s) {
          const uint32_t e = (c.mpack[s / 4] >> (8 * (s % 4))) & 0xffu;
          c.mterm[s] = c.sm + oVec + (e & 63u);
          c.msign[s] = (e & 0x80u) << 24;
        }
        // lane = 8 x + z: the butterfly's stage b subtracts in the lanes with bit b of z set; the phase (-i)^popc(x & z)
        // negates for popc = 2, 3
        c.bflip[0] = (uint32_t)lane << 31;
        c.bflip[1] = ((uint32_t)lane << 30) & 0x80000000u;
        c.bflip[2] = ((uint32_t)lane << 29) & 0x80000000u;
        c.bflip[3] = ((uint32_t)__popc(c.i & c.j) << 30) & 0x80000000u;
      }
    }
  }
  // the butterfly of gsum<G> from stride KK on: for values already summed over aligned groups of KK lanes
  template <int KK>
  __device__ __forceinline__ static double gsum_above(double v) {
    if (KK < 2) v += dpp_f64<0xB1>(v);
    if (KK < 4) v += dpp_f64<0x4E>(v);
    if (G >= 8 && KK < 8) v += dpp_f64<0x141>(v);
    if (G >= 16 && KK < 16) v += dpp_f64<0x140>(v);
    if (G == 64) {
      v += dpp_f64<0x142>(v);
      v += dpp_f64<0x143>(v);
      v = readlane_f64(v, 63);
    }
    return v;
  }
  // The same two butterflies on 32-bit integers: v_add_u32 takes the DPP operand itself, one instruction per level and
  // value where a double takes two moves and an add.
  template <int CTRL>
  __device__ __forceinline__ static uint32_t dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
  }
  template <int KK>
  __device__ __forceinline__ static uint32_t segsum_u32(uint32_t v) {
    v += dpp_u32<0xB1>(v);
    if (KK >= 4) v += dpp_u32<0x4E>(v);
    if (KK >= 8) v += dpp_u32<0x141>(v);
    if (KK >= 16) v += dpp_u32<0x140>(v);
    return v;
  }
  template <int KK>
  __device__ __forceinline__ static uint32_t gsum_above_u32(uint32_t v) {
    if (KK < 2) v += dpp_u32<0xB1>(v);
    if (KK < 4) v += dpp_u32<0x4E>(v);
    if (G >= 8 && KK < 8) v += dpp_u32<0x141>(v);
    if (G >= 16 && KK < 16) v += dpp_u32<0x140>(v);
    if (G == 64) {
      v += dpp_u32<0x142>(v);
      v += dpp_u32<0x143>(v);
      v = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    }
    return v;
  }
  // load_freq of the specialised shape.  A lane knows the R-order slot of each of its rows (Prefetch::ri), so the
  // frequency goes straight there: no parking of the counts in rbuf and no raw[trmap[m]] (two dependent LDS reads)
  // to fetch them back.  The total is the sum of the per-setting sums the shots check forms anyway, continued over the
  // settings: every partial sum is an integer-valued double below 2^53, so any order gives the bits of gsum<G>(part).
  // INTEGER FRONT (n = 3, the kernels with lane tables): where every count of the wavefront lies in [0, 2^22) -- one
  // ballot, wave-uniform -- the per-setting sums and the total are formed as 32-bit integers (216 counts below 2^22: the
  // total is below 2^30) and converted once.  Every number involved is an integer below 2^53, which a double holds
  // exactly: the doubles are those of the sums on doubles, bit for bit.  Anything else takes that path.
  static constexpr bool kIntFront = NQ == 3 && QT_LANE_INT_FRONT != 0;
  template <int LT>
  __device__ static bool load_freq(const CtxSV<LT>& c, const Prefetch& pf) {
    if constexpr (kIntFront && LT != 0) {
      return load_freq_int(c, pf);
    } else {
      double dv[4], st[4];
      bool valid[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        valid[q] = c.l + q * G < c.M;
        dv[q] = valid[q] ? (double)pf.v[q] : 0.0;
        st[q] = segsum_c<d>(dv[q]);
      }
      const double total = gsum_above<d>((st[0] + st[1]) + (st[2] + st[3]));
      const double inv = 1.0 / total;
      bool bad = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) bad |= valid[q] & !shots_match(st[q], total, pf.ns[q], c.a.ns_tot);
      double* fq = c.freq();
      double* dummy = c.rbuf();  // rows beyond M: one slot of a buffer nobody reads before writing it
#pragma unroll
      for (int q = 0; q < 4; ++q) *(valid[q] ? fq + pf.ri[q] : dummy) = dv[q] * inv;
      const unsigned long long votes = __builtin_amdgcn_ballot_w64(bad);
      const int lane = threadIdx.x & 63;
      const unsigned long long mine = (G == 64) ? ~0ull : (((1ull << (G & 63)) - 1ull) << (lane / G * G));
      wave_sync();
      return (votes & mine) == 0ull;
    }
  }
  // (A function of its own, with the statements behind the sums written out a second time: shared with the form above
  // they come out of the compiler in another order there, and k_mle_bfgs and the n = 1, 2 kernels keep their
  // instruction streams, scripts/isa_identity.py.)
  template <int LT>
  __device__ __forceinline__ static bool load_freq_int(const CtxSV<LT>& c, const Prefetch& pf) {
    static_assert(G == 64, "one trial per wavefront");
    double dv[4], st[4], total;
    bool valid[4], small = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      valid[q] = c.l + q * G < c.M;
      small &= (unsigned long long)pf.v[q] < (1ull << 22);
    }
    if (__builtin_amdgcn_ballot_w64(!small) == 0ull) {
      uint32_t is[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t iv = valid[q] ? (uint32_t)pf.v[q] : 0u;
        is[q] = segsum_u32<d>(iv);
        dv[q] = (double)iv;
        st[q] = (double)is[q];
      }
      total = (double)gsum_above_u32<d>((is[0] + is[1]) + (is[2] + is[3]));
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        dv[q] = valid[q] ? (double)pf.v[q] : 0.0;
        st[q] = segsum_c<d>(dv[q]);
      }
      total = gsum_above<d>((st[0] + st[1]) + (st[2] + st[3]));
    }
    const double inv = 1.0 / total;
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) bad |= valid[q] & !shots_match(st[q], total, pf.ns[q], c.a.ns_tot);
    double* fq = c.freq();
    double* dummy = c.rbuf();
#pragma unroll
    for (int q = 0; q < 4; ++q) *(valid[q] ? fq + pf.ri[q] : dummy) = dv[q] * inv;
    wave_sync();
    return __builtin_amdgcn_ballot_w64(bad) == 0ull;
  }

  // ---- factorised contractions for product POVMs -----------------------------------------------
  __device__ __forceinline__ static int ipow(int b, int e) {
    int r = 1;
    for (int q = 0; q < e; ++q) r *= b;
    return r;
  }
  // One stage: out[o] = sum_t tbl(sel, t) * in[base + t * stride], (base, sel) = tab[o].
  // FWD: 4 terms, tbl(sel, t) = tb[sel*4 + t] (row `sel` of the table);  backward: R1 terms,
  // tbl(sel, t) = tb[t*4 + sel] (column `sel`).
  // One output of a contraction stage.  R1C > 0 fixes the table height at compile time (backward
  // stages sum R1 terms): the R1 pairs of LDS reads are then issued together instead of one
  // read-wait-FMA round trip per term, which is what a run-time trip count compiles to.
  template <bool FWD, int R1C = 0>
  __device__ __forceinline__ static double stage_value(const double* tb, int R1, int ent, int stride, const double* in) {
    const int base = ent & 0xffff, sel = ent >> 16;
    if (FWD) {
      const double* row = tb + sel * 4;
      return fma(row[3], in[base + 3 * stride],
                 fma(row[2], in[base + 2 * stride], fma(row[1], in[base + stride], row[0] * in[base])));
    }
    double acc = 0.0;
    if (R1C > 0) {
      double tv[R1C > 0 ? R1C : 1], iv[R1C > 0 ? R1C : 1];
#pragma unroll
      for (int t = 0; t < R1C; ++t) {
        tv[t] = tb[t * 4 + sel];
        iv[t] = in[base + t * stride];
      }
#pragma unroll
      for (int t = 0; t < R1C; ++t) acc = fma(tv[t], iv[t], acc);
      return acc;
    }
    for (int t = 0; t < R1; ++t) acc = fma(tb[t * 4 + sel], in[base + t * stride], acc);
    return acc;
  }
  // All outputs of a stage, two per lane and pass so that their reads overlap.
  template <bool FWD, int R1C, class C>
  __device__ __forceinline__ static void stage_run(const C& c, const double* tb, const int* tab, int n_out, int stride,
                                                   const double* in, double* out) {
    const int R1 = c.R1();
    for (int o = c.l; o < n_out; o += 2 * G) {
      const int o2 = o + G;
      const bool two = o2 < n_out;
      const int e0 = tab[o], e1 = tab[two ? o2 : o];
      const double v0 = stage_value<FWD, R1C>(tb, R1, e0, stride, in);
      const double v1 = stage_value<FWD, R1C>(tb, R1, e1, stride, in);
      out[o] = v0;
      if (two) out[o2] = v1;
    }
  }
  template <bool FWD, class C>
  __device__ static void stage(const C& c, const double* tb, const int* tab, int n_out, int stride, const double* in,
                               double* out) {
    if (FWD) stage_run<true, 0>(c, tb, tab, n_out, stride, in, out);
    else if (c.R1() == 6) stage_run<false, 6>(c, tb, tab, n_out, stride, in, out);
    else if (c.R1() == 4) stage_run<false, 4>(c, tb, tab, n_out, stride, in, out);
    else stage_run<false, 0>(c, tb, tab, n_out, stride, in, out);
    wave_sync();
  }
  template <int R1C, class C>
  __device__ __forceinline__ static double stage_last(const C& c, const double* tb, const int* tab, const double* in) {
    return stage_value<false, R1C>(tb, c.R1(), tab[c.l], 1 << (2 * (NQ - 1)), in);
  }
  // ---- the same stages for a paired table (ProductView::pairedT / pairedP, R1 = 6) ----------------------------
  // Row r = 2a, 2a+1 of such a table is (u_r, 0 .. v_r .. 0) with v_r in column a+1, so a forward output has two
  // terms and a backward output two (k = a+1) or six (k = 0).  The terms that are left are those of stage_value in
  // its order, with coefficients of the same bits (ProductView::cT / cP): what is dropped is fma(0, x, acc) = acc,
  // so the results agree bit for bit, the sign of a zero excepted.  A stage works on its bases
  // (r_1 .. r_(q-1), k_rest), one per lane and indexed in closed form: 6^(q-1) 4^(n-q) <= G of them.
  __device__ __forceinline__ static int paired_bases(int q) { return ipow(6, q - 1) << (2 * (NQ - q)); }
  // forward stage q < n: the base's four inputs make its six outputs
  template <class C>
  __device__ __forceinline__ static void paired_forward(const C& c, int q, const double* in, double* out) {
    const int lk = 2 * (NQ - q), Kq = 1 << lk;
    if (c.l < paired_bases(q)) {
      const int rpre = c.l >> lk, krest = c.l & (Kq - 1);
      const double* ib = in + ((rpre * 4) << lk) + krest;
      double* ob = out + ((rpre * 6) << lk) + krest;
      const double x0 = ib[0];
      const double xa[3] = {ib[Kq], ib[2 * Kq], ib[3 * Kq]};
#pragma unroll
      for (int r = 0; r < 6; ++r) ob[r * Kq] = fma(c.cT(2 * r + 1), xa[r >> 1], c.cT(2 * r) * x0);
    }
    wave_sync();
  }
  // backward stage q >= 2: the base's six inputs make its four outputs
  template <bool PINV, class C>
  __device__ __forceinline__ static void paired_backward(const C& c, int q, const double* in, double* out) {
    const int lk = 2 * (NQ - q), Kq = 1 << lk;
    if (c.l < paired_bases(q)) {
      const int rpre = c.l >> lk, krest = c.l & (Kq - 1);
      const double* ib = in + ((rpre * 6) << lk) + krest;
      double* ob = out + ((rpre * 4) << lk) + krest;
      double y[6], acc = 0.0;
#pragma unroll
      for (int t = 0; t < 6; ++t) y[t] = ib[t * Kq];
#pragma unroll
      for (int t = 0; t < 6; ++t) acc = fma(PINV ? c.cP(2 * t) : c.cT(2 * t), y[t], acc);
      ob[0] = acc;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double v0 = PINV ? c.cP(4 * a + 1) : c.cT(4 * a + 1);
        const double v1 = PINV ? c.cP(4 * a + 3) : c.cT(4 * a + 3);
        ob[(a + 1) * Kq] = fma(v1, y[2 * a + 1], v0 * y[2 * a]);
      }
    }
    wave_sync();
  }

  // Backward pass from Y_n (R-order, in `yn`) to the lane's Y_0[k = l]; PINV: with pinv(T) (A^+ f), else T (A^T y).
  // Intermediates ping-pong between bufB and rbuf; `yn` itself is only read.
  template <bool PINV, class C>
  __device__ static double prod_backward(const C& c, const double* yn) {
    const double* tb = PINV ? c.tabP() : c.tabT();
    const double* in = yn;
    double* bufs[2] = {c.bufB(), c.rbuf()};
    int which = 0;
    if (PINV ? c.pairedP() : c.pairedT()) {
#pragma unroll
      for (int q = NQ; q >= 2; --q) {
        paired_backward<PINV>(c, q, in, bufs[which]);
        in = bufs[which];
        which ^= 1;
      }
      // stage 1 keeps its shape (one output per lane, the table column from LDS); its entry is (k_rest, k_1)
      const int lk = 2 * (NQ - 1);
      return stage_value<false, 6>(tb, 6, (c.l & ((1 << lk) - 1)) | (c.l >> lk) << 16, 1 << lk, in);
    }
    if constexpr (C::kGeneric) {
      const int R1 = c.R1();
      const int* tab = c.tbwd;
#pragma unroll
      for (int q = NQ; q >= 2; --q) {
        const int stride = 1 << (2 * (NQ - q));             // 4^(n-q)
        const int n_out = ipow(R1, q - 1) * 4 * stride;
        stage<false>(c, tb, tab, n_out, stride, in, bufs[which]);
        tab += n_out;
        in = bufs[which];
        which ^= 1;
      }
      // stage 1: D outputs, one per lane
      if (R1 == 6) return stage_last<6>(c, tb, tab, in);
      if (R1 == 4) return stage_last<4>(c, tb, tab, in);
      return stage_last<0>(c, tb, tab, in);
    } else {
      return 0.0;  // (not reached: both tables of the specialised shape are paired)
    }
  }
  // One term of sum freq log p: the eager form (stage_n_log) and the deferred one (deferred_value) both accumulate
  // through this expression, so that both contract to the same fma.
  __device__ __forceinline__ static void add_log_term(double& fpart, double f, double l) { fpart += f * l; }
  // What a deferred first evaluation keeps per lane: p of its rows (two per pass of stage_n_log over the 6^n rows of
  // the specialised shape) and whether any valid row is outside fast_log's regular branch.
  static constexpr int kLogPasses = ((NQ == 1 ? 6 : NQ == 2 ? 36 : 216) + 2 * G - 1) / (2 * G);
  struct DeferredValue {
    double p[2 * kLogPasses];
    bool special;
  };
  // Forward stage n fused with the log-likelihood terms: p = d w (.) X_n + 1e-10, the lane's share of
  // sum freq log p (returned), and Y_n = w (.) freq / p into `rb` (A'^T r = K^T (w (.) r)).  Two outputs per pass
  // so that their LDS round trips (table entry -> operands) overlap; the second of a pair is a recomputation of
  // the first when the row count runs out, and is not stored.
  // PAIRED (ProductView::pairedT): a row keeps its lane -- the order of the sum over rows is part of the value's
  // bits -- and reads its two non-zero coefficients and their operands through the entries of ProductView::last.
  // UNI: equal shots, every row weight is wuni (the same division as wrowR[m]).
  // DEFER (specialised kernels, first evaluation of a trial): no logarithms; the p of this lane's rows are kept in
  // `dv` for deferred_value, with the flag "a valid row would take fast_log's special-case branch".  p and rb[] are
  // formed by the same statements either way.  The specialised shape has M = 6^n rows, so the passes are counted at
  // compile time and p[] stays in registers.
  template <bool PAIRED, bool UNI, bool DEFER = false, class C>
  __device__ __forceinline__ static double stage_n_log(const C& c, const int* tab, const double* in, const double* fr,
                                                       double* rb, DeferredValue* dv = nullptr) {
    const double* tb = c.tabT();
    auto x_of = [&](int ent) {
      if (!PAIRED) return stage_value<true>(tb, c.R1(), ent, 1, in);
      const int vi = ent >> 16;
      return fma(tb[vi], in[(ent >> 8) & 0xff], tb[vi & ~3] * in[ent & 0xff]);
    };
    auto w_of = [&](int o) {
      if constexpr (UNI) return c.wuni();
      else return c.twrow[o];
    };
    double fpart = 0.0;
    bool special = false;
    auto pass = [&](int o, int s) {
      const int o2 = o + G;
      const bool two = o2 < c.M;
      const int oo = two ? o2 : o;
      const int e0 = tab[o], e1 = tab[oo];
      const double x0 = x_of(e0), x1 = x_of(e1);
      const double w0 = w_of(o), w1 = w_of(oo);
      const double f0 = fr[o], f1 = fr[oo];
      const double p0 = x0 * w0 * d + 1e-10, p1 = x1 * w1 * d + 1e-10;
      if constexpr (DEFER) {
        dv->p[2 * s] = p0;
        dv->p[2 * s + 1] = p1;
        special |= !log_is_regular(p0);
      } else {
        const double l0 = fast_log(p0), l1 = fast_log(p1);
        add_log_term(fpart, f0, l0);
        if (two) add_log_term(fpart, f1, l1);
      }
      rb[o] = w0 * f0 * recip_nr(p0);
      if (two) {
        if constexpr (DEFER) special |= !log_is_regular(p1);
        rb[o2] = w1 * f1 * recip_nr(p1);
      }
    };
    if constexpr (DEFER) {
#pragma unroll
      for (int s = 0; s < kLogPasses; ++s) {
        const int o = c.l + s * 2 * G;
        dv->p[2 * s] = dv->p[2 * s + 1] = 1.0;
        if (o < c.M) pass(o, s);
      }
      dv->special = special;
    } else {
      for (int o = c.l; o < c.M; o += 2 * G) pass(o, 0);
    }
    return fpart;
  }
  // -sum freq log p of a deferred first evaluation: the terms of stage_n_log in its row order, through the same
  // add_log_term.  Executed by every lane of the wavefront; freq[] is still what stage_n_log read.
  template <class C>
  __device__ __forceinline__ static double deferred_value(const C& c, const DeferredValue& dv) {
    const double* fr = c.freq();
    double fpart = 0.0;
#pragma unroll
    for (int s = 0; s < kLogPasses; ++s) {
      const int o = c.l + s * 2 * G;
      if (o < c.M) {
        const int o2 = o + G;
        const bool two = o2 < c.M;
        const double f0 = fr[o], f1 = fr[two ? o2 : o];
        const double l0 = fast_log(dv.p[2 * s]), l1 = fast_log(dv.p[2 * s + 1]);
        add_log_term(fpart, f0, l0);
        if (two) add_log_term(fpart, f1, l1);
      }
    }
    return -gsum<G>(fpart);
  }
  // The value of a deferred first evaluation where something reads it: `wanted` (the trial goes on to BFGS, or the
  // caller asked for `fun`) or a p outside fast_log's regular branch, where the value may be a NaN and status 4 asks.
  // Decided per wavefront: every lane runs the reduction or none does.  Otherwise 0: with every p positive and
  // finite the value is no NaN unless a frequency is one, and then the gradient norm is a NaN as well.
  template <class C>
  __device__ __forceinline__ static double value_if_needed(const C& c, const DeferredValue& dv, bool wanted) {
    if (!__any(wanted || dv.special)) return 0.0;
    const double f = deferred_value(c, dv);
    QT_STAMP(19);
    return f;
  }
  // sum_m Op[m][lane] * vec[m]   (lane = column)
  template <class C>
  __device__ __forceinline__ static double col_dot(const C& c, const double* g_rowmajor, const double* vec) {
    return dot_global<16>(g_rowmajor, D, (unsigned)c.l, vec, c.M);
  }
  // sum_k Op[row][k] * vec[k]    (lane = row), g_transposed = [D][M]
  template <class C>
  __device__ __forceinline__ static double row_dot(const C& c, const double* g_transposed, int row, const double* vec) {
    return dot_global<(D < 16 ? D : 16)>(g_transposed, (size_t)c.M, (unsigned)row, vec, D);
  }

  // ---- a6: linear inversion (operand PinvT).  Returns lane's element of rho; vec() = Bloch vector.
  template <class C>
  __device__ static cd lin_invert(const C& c, double& bloch_l) {
    if constexpr (!C::kGeneric) {
      bloch_l = prod_backward<true>(c, c.freq()) / (c.wuni() * d);
    } else if (c.prod()) {
      if (c.uniform()) {
        // pinv(w K) = pinv(T)^(x n) / w : the same backward pass with pinv(T) instead of T
        bloch_l = prod_backward<true>(c, c.freq()) / (c.wuni() * d);
      } else {  // unequal shots per setting: dense left inverse, rows visited in R-order
        double acc = 0.0;
        for (int m = 0; m < c.M; ++m) acc = fma(c.pv.PinvT[(size_t)c.trmap[m] * D + c.l], c.freq()[m], acc);
        bloch_l = acc / d;
      }
    } else {
      bloch_l = col_dot(c, c.pv.PinvT, c.freq()) / d;  // bloch_k = sum_m Pinv[k][m] f_m / d
    }
    c.vec()[c.l] = bloch_l;
    wave_sync();
    cd r = matrix_of(c, c.vec());
    wave_sync();
    return r;
  }

  // ---- the parallel-order cyclic Jacobi eigensolver behind a7 and the trace distance / infidelity.
  // In: lane's element of a Hermitian matrix A (real diagonal) and of V (the identity, or a basis to carry along).
  // Out: A' = J^dagger A J with its eigenvalues on the diagonal lanes, V' = V J.
  // Round r = 1 .. d-1 rotates the d/2 disjoint pairs (k, k ^ r): every pair once per sweep.  A
  // round is ONE LDS round trip: the lanes publish A and V, then each lane reads the two 2x2
  // blocks that define the rotations of its column pair {j, j^r} and row pair {i, i^r} together
  // with its three partner elements, and applies A' = J^dagger A J, V' = V J in registers.
  // The loop is left when no lane group of the wavefront has off^2 > jtol2 * ||A||_F^2 (a NaN compares false: such a
  // matrix is never rotated), after 20 sweeps at the latest.
  // OWN: a group whose own matrix has met the rule keeps its registers while its wavefront neighbours go on, so that a
  // trial's bits depend on nothing but the trial (n = 3: one trial per wavefront, no difference).
  // VEC = false: eigenvalues only, V is neither read nor written.
  template <bool OWN = false, bool VEC = true, class C>
  __device__ __forceinline__ static void jacobi_sweeps(const C& c, cd& a_io, cd& v_io) {
    // (the loop runs on values of its own: on the caller's two objects three callers of psd_project allocate a register
    // differently from the loop written out in psd_project)
    cd a = a_io, v = v_io;
    const int i = c.i, j = c.j;
    cd* const Ai = c.A();
    cd* const Vi = c.V();
    const double nrm = gsum<G>(a.re * a.re + a.im * a.im);  // Frobenius norm: invariant
    for (int sweep = 0; sweep < 20; ++sweep) {
      const double off = gsum<G>(i != j ? a.re * a.re + a.im * a.im : 0.0);
      const bool met = !(off > c.jtol2() * nrm);  // this group's own matrix
      if (__all(met)) break;
#pragma unroll 1
      for (int r = 1; r < d; ++r) {
        Ai[c.e] = a;
        if constexpr (VEC) Vi[c.e] = v;
        wave_sync();
        const int pj = j ^ r, pi = i ^ r;
        const int cp = j < pj ? j : pj, cq = j < pj ? pj : j;  // column pair, ordered
        const int rp = i < pi ? i : pi, rq = i < pi ? pi : i;  // row pair, ordered
        const double c_pp = Ai[cp * LD + cp].re, c_qq = Ai[cq * LD + cq].re;
        const cd c_pq = Ai[cp * LD + cq];
        const double r_pp = Ai[rp * LD + rp].re, r_qq = Ai[rq * LD + rq].re;
        const cd r_pq = Ai[rp * LD + rq];
        const cd a_c = Ai[i * LD + pj], a_r = Ai[pi * LD + j], a_x = Ai[pi * LD + pj];
        cd v_c{0.0, 0.0};
        if constexpr (VEC) v_c = Vi[i * LD + pj];
        wave_sync();  // all reads of this image are issued before the next round overwrites it
        double cj, ci;
        cd wj, wi;
        rotation(c_pp, c_qq, c_pq, cj, wj);
        rotation(r_pp, r_qq, r_pq, ci, wi);
        if (j < pj) wj = cd{-wj.re, wj.im};  // J[pj][j]: -conj(w) if j is the lower index, else w
        if (i < pi) wi = cd{-wi.re, wi.im};
        // A'_ij = ci (a_ij cj + a_i,pj wj) + conj(wi) (a_pi,j cj + a_pi,pj wj) ;  V' = V J
        const cd t0 = cadd(cscale(a, cj), cmul(a_c, wj));
        const cd t1 = cadd(cscale(a_r, cj), cmul(a_x, wj));
        const cd an = cadd(cscale(t0, ci), cmulc(t1, wi));
        if (!(OWN && G < 64 && met)) {
          a = an;
          if constexpr (VEC) v = cadd(cscale(v, cj), cmul(v_c, wj));
        }
        if (i == j) a.im = 0.0;
      }
    }
    a_io = a;
    v_io = v;
  }

  // ---- a7: eigenvalue clip + trace renormalisation.
  // In: lane's element of a Hermitian matrix.  Out: lane's element of U max(v, eps) U^dagger / Tr.
  template <class C>
  __device__ static cd psd_project(const C& c, cd a, double eps) {
    const int i = c.i, j = c.j;
    cd* Vi = c.V();
    cd v{i == j ? 1.0 : 0.0, 0.0};
    if (i == j) a.im = 0.0;
    jacobi_sweeps(c, a, v);
    // rebuild with clipped eigenvalues: R_ij = sum_k V_ik max(lam_k, eps) conj(V_jk)
    double* lam = c.lam();
    Vi[c.e] = v;
    if (i == j) lam[i] = a.re;
    wave_sync();
    cd rr{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) {
      const double lc = lam[k] > eps ? lam[k] : eps;  // np.maximum(eps, v)
      const cd p = cmulc(Vi[i * LD + k], Vi[j * LD + k]);
      rr.re += lc * p.re;
      rr.im += lc * p.im;
    }
    const double tr = gsum<G>(i == j ? rr.re : 0.0);
    wave_sync();
    return cd{rr.re / tr, rr.im / tr};
  }

  // ---- trace distance and infidelity (geometry.py:23-38, 41-56) of Hermitian matrices, by the sweeps above: both are
  // symmetric functions of the eigenvalues of ONE Hermitian matrix per trial.  No POVM is read and the scratch of a lane
  // group is two matrix images, so these have a context of their own (k_psd_sqrt, k_metric_dist).
  static constexpr int kMetricDoubles = 2 * MAT;  // per trial: images X / A and Y / V
  struct CtxM {
    int l, i, j, e;
    double* sm;
    double tol2;
    __device__ __forceinline__ cd* A() const { return reinterpret_cast<cd*>(sm); }
    __device__ __forceinline__ cd* V() const { return reinterpret_cast<cd*>(sm + MAT); }
    __device__ __forceinline__ double jtol2() const { return tol2; }
  };
  __device__ __forceinline__ static void make_ctx_metric(CtxM& c, double* smem_block, double jtol2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    c.l = lane % G;
    c.i = c.l / d;
    c.j = c.l % d;
    c.e = c.i * LD + c.j;
    c.sm = smem_block + (wave * TPW + lane / G) * kMetricDoubles;
    c.tol2 = jtol2;
  }
  // What a distance becomes when its matrix holds a NaN or an infinity (the sweeps never rotate such a matrix, so its
  // diagonal says nothing): n2 = the squared Frobenius norm of the matrix the sweeps were given.
  __device__ __forceinline__ static double finite_or_nan(double n2, double val) {
    return n2 < __builtin_inf() ? val : __builtin_nan("");
  }
  // geometry.py:23-38 for Hermitian arguments: |Tr sqrt(Delta^2)| / 2 = sum_i |lambda_i(Delta)| / 2, Delta = R - C with
  // the imaginary parts of its diagonal dropped (as psd_project drops them); 0 below 1e-15.  In: the lane's elements of
  // R and C.  Every lane of the group returns the same bits.
  template <class C>
  __device__ static double trace_dist(const C& c, cd r, cd cen) {
    cd a{r.re - cen.re, c.i == c.j ? 0.0 : r.im - cen.im}, v{0.0, 0.0};
    const double n2 = gsum<G>(a.re * a.re + a.im * a.im);
    jacobi_sweeps<true, false>(c, a, v);
    const double val = 0.5 * gsum<G>(c.i == c.j ? fabs(a.re) : 0.0);
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }
  // The Hermitian root of a Hermitian matrix with its negative eigenvalues clipped to 0: sum_k V_ik sqrt(max(lam_k, 0))
  // conj(V_jk), real on the diagonal.  NaN throughout for a matrix that holds a NaN or an infinity.
  template <class C>
  __device__ static cd psd_sqrt(const C& c, cd a) {
    const int i = c.i, j = c.j;
    cd* Ai = c.A();
    cd* Vi = c.V();
    cd v{i == j ? 1.0 : 0.0, 0.0};
    if (i == j) a.im = 0.0;
    const double n2 = gsum<G>(a.re * a.re + a.im * a.im);
    jacobi_sweeps<true>(c, a, v);
    Ai[c.e] = a;
    Vi[c.e] = v;
    wave_sync();
    cd rr{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) {
      const double lam = Ai[k * LD + k].re;
      const double w = sqrt(lam > 0.0 ? lam : 0.0);
      const cd p = cmulc(Vi[i * LD + k], Vi[j * LD + k]);
      rr.re += w * p.re;
      rr.im += w * p.im;
    }
    wave_sync();
    if (i == j) rr.im = 0.0;
    return cd{finite_or_nan(n2, rr.re), finite_or_nan(n2, rr.im)};
  }
  // geometry.py:41-56 for Hermitian arguments: 1 - (Tr sqrt(S R S))^2 = 1 - (sum_i sqrt(max(mu_i, 0)))^2 with S = sqrt(C)
  // (psd_sqrt; fidelity is symmetric, so the root of the centre stands in for the reference's root of its first
  // argument) and mu the eigenvalues of the Hermitian part of M = S R S; 0 below 1e-15, small negatives included.
  // In: the lane's elements of R and S.  M is formed by two d x d products through the group's two images.
  template <class C>
  __device__ static double infidelity(const C& c, cd r, cd s) {
    const int i = c.i, j = c.j;
    cd* X = c.A();
    cd* Y = c.V();
    X[c.e] = s;
    Y[c.e] = r;
    wave_sync();
    cd t{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) t = cadd(t, cmul(X[i * LD + k], Y[k * LD + j]));  // T = S R
    wave_sync();
    Y[c.e] = t;
    wave_sync();
    cd m{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) m = cadd(m, cmul(Y[i * LD + k], X[k * LD + j]));  // M = T S
    wave_sync();
    const int src = (int)(threadIdx.x & 63) - c.l + j * d + i;  // the lane of element (j, i)
    const cd mt{__shfl(m.re, src, 64), __shfl(m.im, src, 64)};
    cd a{0.5 * (m.re + mt.re), i == j ? 0.0 : 0.5 * (m.im - mt.im)}, v{0.0, 0.0};
    const double n2 = gsum<G>(a.re * a.re + a.im * a.im);
    jacobi_sweeps<true, false>(c, a, v);
    const double rf = gsum<G>(i == j ? sqrt(a.re > 0.0 ? a.re : 0.0) : 0.0);
    const double val = 1.0 - rf * rf;
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }

  // ---- a8: lower Cholesky factor of the matrix whose element this lane holds.
  // Leaves L in Bm() (upper part zero) and returns the lane's parameter x_l; ok = 0 if not PD.
  // The elimination is carried on past a non-positive pivot as L S L^dagger (S = signs), so that by
  // Sylvester's law `neg` is the number of negative eigenvalues (99 when a pivot is too small for
  // the count to mean anything) and `kneg` the first index where the leading block stops being PD.
  // SPEC (latency-bound launches only: one wave per SIMD, the fused kernel): the Gauss-Jordan inverse that
  // lift_single_negative needs when the LAST pivot is the negative one (kneg = d - 1, the generic case for one small
  // negative eigenvalue: natural pivot order) runs in the same sweep, step k of it beside step k of the elimination --
  // two independent dependency chains sharing the LDS round trips.  A trial that turns out not positive definite then
  // skips ~3 k of its ~39 k clocks (the launch ends with its slowest wave, and those are the clipped trials); a
  // positive definite one throws the inverse away, ~1.5 k clocks it had to spare.  Same arithmetic, same bits, as the
  // loop in lift_single_negative.  *spec_inv = this lane's element of the inverse (garbage unless kneg = d - 1).
  // (k_mle_fused_hw runs the plain sweep: there the trial's helper wavefront speculates, see HelperLink.)
  template <bool SPEC = false, class C>
  __device__ static double cholesky_param(const C& c, cd a, int& ok, int* neg_out = nullptr, int* kneg_out = nullptr,
                                          cd* spec_inv = nullptr) {
    cd* A = c.A();
    cd* L = c.Bm();
    cd* Vs = c.V();
    const int i = c.i, j = c.j;
    A[c.e] = a;
    int neg = 0, kneg = d - 1;
    cd lmine{0.0, 0.0};  // this lane's element of L (its column j is final after step k = j)
    cd b = a;            // SPEC: the matrix on its way to its inverse
    if (SPEC && i == j) b.im = 0.0;
    if (SPEC) Vs[c.e] = b;
    wave_sync();
#pragma unroll
    for (int k = 0; k < d; ++k) {
      // The pivot sits in the register of lane (k, k): with one trial per wave it is taken from there
      // (v_readlane), so that 1/sqrt runs while the column is still on its way through LDS.
      const double akk = (G == 64) ? readlane_f64(a.re, k * d + k) : A[k * LD + k].re;
      const cd aik = A[i * LD + k], ajk = A[j * LD + k];
      if constexpr (SPEC) {  // step p = k of the inverse (lift_single_negative's loop body)
        const double piv = readlane_f64(b.re, k * d + k);
        const cd bip = Vs[i * LD + k], bpj = Vs[k * LD + j];
        double inv = __builtin_amdgcn_rcp(piv);
        inv = fma(inv, fma(-piv, inv, 1.0), inv);
        inv = fma(inv, fma(-piv, inv, 1.0), inv);
        const cd t{bpj.re * inv, bpj.im * inv};
        const cd e = cmul(bip, t);
        cd nb{b.re - e.re, b.im - e.im};
        if (j == k) nb = cd{-bip.re * inv, -bip.im * inv};
        if (i == k) nb = (j == k) ? cd{inv, 0.0} : t;
        b = nb;
        if (k + 1 < d) Vs[c.e] = b;  // published by the elimination's wave_sync below
      }
      const double mag = fabs(akk);
      const bool pos = akk > 0.0;
      if (!pos) {
        if (neg == 0) kneg = k;
        ++neg;
      }
      if (!(mag > 1e-13)) neg = neg > 0 ? 99 : neg;  // NaN lands here too
      // In the sweep only 1 / a_kk is needed (a_ij -= s a_ik conj(a_jk) / |a_kk|); the square roots that turn
      // the columns into L are taken once, for all columns in parallel, after the sweep.
      const double safe = mag > 1e-300 ? mag : 1e-300;
      if (k + 1 < d) {
        const double inv = recip_nr(safe);
        const double sinv = pos ? -inv : inv;
        const cd ajs{ajk.re * sinv, ajk.im * sinv};  // -s a_jk / |a_kk|
        const bool upd = i > k && j > k;
        const double nre = fma(aik.re, ajs.re, fma(aik.im, ajs.im, a.re));
        const double nim = fma(aik.im, ajs.re, fma(-aik.re, ajs.im, a.im));
        a.re = upd ? nre : a.re;
        a.im = upd ? nim : a.im;
        A[c.e] = a;  // branch-free: lanes outside the trailing block store their old value again
        wave_sync();
      }
    }
    {
      // lane (i, j), i >= j: its register still holds a_ij as it was when column j became the pivot column
      const double dj = A[j * LD + j].re;
      const double mj = fabs(dj);
      const double rs = fast_rsqrt(mj > 1e-300 ? mj : 1e-300);  // 1 / |l_jj|
      if (i >= j) lmine = (i == j) ? cd{dj * rs, 0.0} : cd{a.re * rs, a.im * rs};
    }
    ok = neg == 0;
    if (neg_out) *neg_out = neg;
    if (kneg_out) *kneg_out = kneg;
    if (SPEC && spec_inv) *spec_inv = b;
    L[c.e] = lmine;
    wave_sync();
    const cd e = L[c.pi * LD + c.pj];
    const double x = c.pkind == 2 ? e.im : e.re;
    wave_sync();
    return x;
  }

  // ---- k_mle_fused_hw (n = 3): the hand-off between a trial's wavefront and its twin wavefront on the same SIMD.
  // Between lin_invert and the lifted matrix a clipped trial is one serial chain (first Cholesky sweep, Gauss-Jordan
  // inverse, squarings, certificate), and nothing of the lift needs the sweep except the knowledge that the lift is
  // wanted.  So the twin (the "helper" below) runs lift_single_negative in natural pivot order on EVERY trial,
  // speculatively, while the trial's wave runs the plain sweep; the verdict of the sweep then lets it go on or sends
  // it home.  The twin is given nothing: it reads the trial's counts itself and runs load_freq and lin_invert on a
  // scratch of its own (behind the scratches of the workgroup's four trials), so the matrix it lifts is in its own
  // registers, bit for bit the trial's, at the moment the trial's sweep starts, and the lift's two images are the A()
  // and V() of that scratch.  After "go" the twin KEEPS the lifted matrix in its registers and goes on as the trial --
  // first evaluation, outputs, BFGS loop, all on its own context -- and the wave on threadIdx.y = 0 becomes the
  // helper: it receives the matrix and runs the second Cholesky sweep of it (L into the twin's Bm()) while the twin
  // runs the front of the first nll_grad (the two are independent).  One wave owns a trial's outputs; the
  // compare-and-swap on `verdict` decides which (strictly so as long as no count runs out: see await_lift for the
  // one branch behind a claimed verdict where both waves would go on as the trial).  In the names and comments of
  // HelperLink, "the trial's wave" is the wave on threadIdx.y = 0 up to kLifted and the twin behind it, and "the
  // helper" is the other one: the role swaps with the ownership.  What crosses between the waves goes through the first doubles of the
  // trial's LDS pair store (TwoLoop::lp, which nothing touches before the BFGS loop): the lifted matrix,
  // the parameters of the sweep and the words below.
  // Data first, then the flag: release stores and acquire loads at workgroup scope, no workgroup barrier besides the
  // one of make_ctx -- the four trials of a workgroup stay uncoupled.  Every wait is a counted loop; whoever runs out
  // of polls leaves:
  //   trial:  after its sweep, `verdict`:
  //           kAbort (positive definite: it never waits; or a class the natural-order lift does not serve: wrong
  //           pivot, several negative pivots -- today's serial code on its own wave) or kGo (one negative pivot, the
  //           last).  After kGo it polls `lifted`: kLifted -> the matrix is in result() and the trial is the twin's:
  //           this wave runs sweep_for (second sweep, L into the twin's Bm(), which the front of an evaluation with a
  //           StartPoint does not touch; x, ok, done), publishes `gone` and leaves without writing an output;
  //           kRefused -> it stays the trial and runs the eigensolver on its own wave (the lift on its own wave would
  //           refuse with the same bits).  Out of polls: it takes the verdict back (compare-and-swap kGo -> kRevoked: a
  //           twin that has not claimed it never will) and runs the serial path.  If the twin had claimed it, the twin
  //           is inside straight-line code that waits for nobody, and a second, much longer count covers that many
  //           times over.
  //   twin:   runs the lift on its own images, looking at `verdict` once per squaring (CtxH::abandoned) and leaving on
  //           anything but "none yet" or kGo.  At the end it waits for the verdict, claims kGo (-> kClaimed), publishes
  //           kRefused and leaves, or the matrix and kLifted (twin_lift); then it is the trial: nll_grad<.., LATE> with
  //           collect() behind the front, and if x does not come or ok = 0, today's fallbacks on its own wave and its
  //           own `lin`.  Before that it writes nothing outside its own scratch.
  //   `gone` = 1 is the last write of whichever wave leaves; the wave that owns the trial acquires it before the BFGS
  //   loop writes the first pair over this region.
  struct HelperLink {
    enum : int { kPending = 0, kGo = 1, kAbort = 2, kClaimed = 3, kRevoked = 4 };  // verdict
    enum : int { kNothing = 0, kLifted = 1, kRefused = 2 };                  // lifted
    // polls (each an LDS read and an s_sleep): the helper's waits cover the longest path to the verdict (~20 k clocks)
    // several hundred times, the trial's first wait the helper's ~11 k-clock chain likewise
    static constexpr int kHelperPolls = 1 << 15, kWaitPolls = 1 << 14, kClaimedPolls = 1 << 16;
    double* base;  // [MAT] the lifted matrix, [D] x, then the words
    int pending;   // the lifted matrix is the twin's: the twin evaluates it, the other wave factorises it (wave-uniform)
    __device__ __forceinline__ static constexpr int doubles() { return MAT + D + 3; }
    __device__ __forceinline__ cd* result() const { return reinterpret_cast<cd*>(base); }
    __device__ __forceinline__ double* x() const { return base + MAT; }
    __device__ __forceinline__ int* verdict() const { return reinterpret_cast<int*>(base + MAT + D); }
    __device__ __forceinline__ int* lifted() const { return verdict() + 1; }
    __device__ __forceinline__ int* done() const { return verdict() + 2; }
    __device__ __forceinline__ int* gone() const { return verdict() + 3; }
    __device__ __forceinline__ int* ok() const { return verdict() + 4; }
    __device__ __forceinline__ static void publish(int* w, int v) {  // after this wave's data writes
      wave_sync();
      if ((threadIdx.x & 63) == 0) __hip_atomic_store(w, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ static int peek(const int* w) {
      return __builtin_amdgcn_readfirstlane(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    }
    __device__ __forceinline__ static bool claim(int* w, int from, int to) {  // by one lane; the same answer in all
      int won = 0;
      if ((threadIdx.x & 63) == 0) {
        int expect = from;
        won = __hip_atomic_compare_exchange_strong(w, &expect, to, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      return __builtin_amdgcn_readfirstlane(won) != 0;
    }
    template <int SLEEP>
    __device__ __forceinline__ static int poll(const int* w, int idle, int polls) {  // the word once it is not `idle`
      int v = idle;
#pragma unroll 1
      for (int n = 0; n < polls; ++n) {
        v = peek(w);
        if (v != idle) break;
        __builtin_amdgcn_s_sleep(SLEEP);
      }
      return v;
    }
    // trial's wave, before the workgroup barrier of make_ctx (every launch sets its words up: nothing is left over)
    __device__ __forceinline__ void reset() {
      pending = 0;
      if ((threadIdx.x & 63) == 0) {
        *verdict() = kPending;
        *lifted() = kNothing;
        *done() = 0;
        *gone() = 0;
      }
    }
    __device__ __forceinline__ void decide(bool go) const { publish(verdict(), go ? kGo : kAbort); }
    // trial's wave, after decide(true): kLifted = this lane's element of the lifted matrix is in `proj` and the helper
    // is factorising it; kRefused = the lift ran and declined; kNothing = nothing came and nothing will (or, after a
    // claimed verdict and the long count, the helper has stopped making progress).  That last case is the one place
    // where ownership rests on a bounded wait and not on the compare-and-swap: the twin has claimed and, if it is still
    // alive, will publish kLifted and go on as the trial while this wave runs the serial path as the trial too; both
    // would then write the trial's outputs and pairs (the same values, but unsynchronised).  The twin's stretch between
    // its claim and its publish is a store and a release, set against 2^16 polls; as with await_gone, a twin that has
    // not answered by then has stopped making progress.  No test forces it.
    __device__ __forceinline__ int await_lift(int e, cd& proj) {
      int v = poll<1>(lifted(), kNothing, kWaitPolls);
      if (v == kNothing) {
        if (claim(verdict(), kGo, kRevoked)) return kNothing;
        v = poll<1>(lifted(), kNothing, kClaimedPolls);
        if (v == kNothing) return kNothing;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (v == kLifted) {
        proj = result()[e];
        pending = 1;
      }
      return v;
    }
    // trial's wave: the helper's parameters; false = they did not come (the helper claimed the verdict before it
    // published the matrix and waits for nobody behind that: the long count covers its sweep many times over)
    __device__ __forceinline__ bool collect(int l, double& xl, int& okl) const {
      if (poll<1>(done(), 0, kClaimedPolls) == 0) return false;
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      xl = x()[l];
      okl = *ok();
      return true;
    }
    // trial's wave, before the first (s, y) pair goes into the LDS pair store: the helper has left this region.  In any
    // normal run that was thousands of clocks ago and this is one LDS read.  The wait is bounded like every other: after
    // 2^16 polls without an answer the trial's wave goes on and writes its pairs unsynchronised (a helper that has not
    // left by then has stopped making progress; its region is the first pairs', and nothing reads what it wrote).
    __device__ __forceinline__ void await_gone() const {
      poll<1>(gone(), 0, kClaimedPolls);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
  };
  // The twin's view of the images behind lin_invert: A() and V() are those of its own scratch, Bm() is the trial's
  // (cholesky_param leaves L there).  The lane constants are those of its trial context (make_ctx).
  struct CtxH {
    int l, i, j, e, pi, pj, pkind;
    cd *image, *second, *factor;
    const int* verdict;
    __device__ __forceinline__ cd* A() const { return image; }
    __device__ __forceinline__ cd* Bm() const { return factor; }
    __device__ __forceinline__ cd* V() const { return second; }
    // lift_single_negative on speculation: the word is loaded with a batch of LDS reads the lift issues anyway and
    // looked at behind them, so a look costs an issue slot and a scalar compare, not an LDS round trip
    __device__ __forceinline__ int verdict_load() const {
      return __hip_atomic_load(verdict, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ static bool abandoned(int v) {
      v = __builtin_amdgcn_readfirstlane(v);
      return v != HelperLink::kPending && v != HelperLink::kGo;
    }
  };
  // What nll_grad<.., LATE> got from the helper: `got` = it came (otherwise x is a finite stand-in and the caller
  // evaluates again from the top), the parameter of this lane, and whether the matrix was positive definite.
  struct LateX {
    bool got;
    double x;
    int ok;
  };
  // The context of a trial's wavefront in k_mle_fused_hw: that of k_mle_fused, and the link to its helper.
  template <class Base>
  struct WithHelper : Base {
    HelperLink* link;
    LateX* late;    // nll_grad<.., LATE>
    double* xtra;   // the trial's `extra` doubles: behind the trial's scratch, for the twin too (whose own scratch has none)
    __device__ __forceinline__ double* extra() const { return xtra; }
    static constexpr bool kHelper = true;
  };
  __device__ __forceinline__ static void param_owner(int l, int& pi, int& pj, int& pkind) {
    // parameter l: diagonal (l, l), then the T real and the T imaginary parts in the order of np.tril_indices(d, -1);
    // row ii of entry t is the number of triangular numbers k (k - 1) / 2 <= t, k = 1 .. d - 1
    const bool diag = l < d, imag = l >= d + T;
    const int t = l - d - (imag ? T : 0);
    int ii = 1;
#pragma unroll
    for (int k = 2; k < d; ++k) ii += t >= (k * (k - 1)) / 2;
    pkind = diag ? 0 : imag ? 2 : 1;
    pi = diag ? l : ii;
    pj = diag ? l : t - (ii * (ii - 1)) / 2;
  }
  // The twin behind lin_invert: `t` its own trial context, `lin` its own linear-inversion matrix.  True: it has lifted,
  // claimed the verdict and published the lifted matrix, whose element of this lane is `proj` -- from here on it IS the
  // trial (it holds the counts' frequencies, the context and the matrix) and the wave on threadIdx.y = 0 is its helper
  // (sweep_for).  False: it leaves, and the caller publishes `gone`.
  template <class C>
  __device__ static bool twin_lift(const C& t, const HelperLink& k, cd lin, cd& proj) {
    static_assert(G == 64, "one trial per wavefront");
    CtxH c = side_ctx(t, k, t.Bm());
    proj = cd{0.0, 0.0};
    const bool lifted = __builtin_amdgcn_readfirstlane((int)lift_single_negative<true>(c, lin, d - 1, 1e-15, proj, nullptr)) != 0;
    QT_STAMP(6);
    // (an abandoned lift finds its kAbort here at the first look)
    if (HelperLink::template poll<1>(k.verdict(), HelperLink::kPending, HelperLink::kHelperPolls) != HelperLink::kGo) return false;
    QT_STAMP(7);
    if (!HelperLink::claim(k.verdict(), HelperLink::kGo, HelperLink::kClaimed)) return false;
    if (!lifted) {
      HelperLink::publish(k.lifted(), HelperLink::kRefused);
      return false;
    }
    k.result()[c.e] = proj;
    HelperLink::publish(k.lifted(), HelperLink::kLifted);
    return true;
  }
  // The wave on threadIdx.y = 0 after kLifted: the second Cholesky sweep of the lifted matrix, on its own A(), with L
  // going into the twin's Bm() `L` (the front of the twin's evaluation does not touch it); then x, ok, done.
  template <class C>
  __device__ static void sweep_for(const C& t, const HelperLink& k, cd proj, cd* L) {
    CtxH c = side_ctx(t, k, L);
    int ok2;
    const double x2 = cholesky_param(c, proj, ok2);
    k.x()[c.l] = x2;
    if (c.l == 0) *k.ok() = ok2;  // (wave-uniform: the pivots are read from their lanes)
    HelperLink::publish(k.done(), 1);
    QT_STAMP(7);
  }
  template <class C>
  __device__ __forceinline__ static CtxH side_ctx(const C& t, const HelperLink& k, cd* L) {
    CtxH c;
    c.l = t.l;
    c.i = t.i;
    c.j = t.j;
    c.e = t.e;
    c.pi = t.pi;
    c.pj = t.pj;
    c.pkind = t.pkind;
    c.image = t.A();
    c.second = t.V();
    c.factor = L;
    c.verdict = k.verdict();
    return c;
  }

  // ---- a7, short cut for exactly ONE negative eigenvalue (lam_1 < 0 < lam_2 <= ...):
  //   U max(v, eps) U^dagger = A + (eps - lam_1) v_1 v_1^dagger,
  // so only the projector N = v_1 v_1^dagger is needed.  M = A^{-1} (Gauss-Jordan, pivot order with
  // `kneg` last: the leading block is positive definite, so no pivoting is needed) has v_1 as its
  // dominant direction whenever |lam_1| < lam_2; N <- N N^dagger / Tr squares the separation
  // ratio each time (k squarings = 2^k inverse-iteration steps at the cost of k 8x8 products).
  // Certified, not assumed: purity Tr N^2 -> 1 (then one more squaring: contamination < 1e-14),
  // lam_1 = Tr(A N) < eps, and ||A N - lam_1 N||_F <= 1e-13 ||A||_F.  Returns false (caller runs the
  // Jacobi eigensolver on the untouched input) on a slow ratio, a positive lam, or a failed check.
  // `inverse`: the lane's element of A^{-1} when the caller already has it (cholesky_param<true>, kneg = d - 1).
  // One function for the trial's wavefront and for the helper wavefront of k_mle_fused_hw, which runs it before anybody
  // knows whether it is wanted and returns false behind the squaring in which C::abandoned says it is not (HelperLink).
  // NATURAL: the caller's kneg is d - 1 at compile time (the twin of k_mle_fused_hw: the natural pivot order 0 .. d - 1).
  // The d steps are then unrolled: the pivot comes from a constant lane, the LDS offsets of row and column p are
  // immediates, and the step counter, its compare and its branch are gone.  The arithmetic of a step is the same text.
  // `out` is written whenever the squarings certify, also when the checks behind them refuse (kLiftOneExit): a caller
  // reads it only behind `true`.
  template <bool NATURAL = false, class C>
  __device__ static bool lift_single_negative(const C& c, cd r, int kneg, double eps, cd& out,
                                              const cd* inverse = nullptr) {
    static_assert(G == 64, "one trial per wavefront: the flags below are wave-uniform");
    cd* Ai = c.A();
    cd* Vi = c.V();
    const int i = c.i, j = c.j;
    if (i == j) r.im = 0.0;
    cd b = r;
    if (inverse) b = *inverse;
    auto eliminate = [&](int p) {  // one Gauss-Jordan step on pivot p
      Ai[c.e] = b;
      const double piv = readlane_f64(b.re, p * d + p);  // from lane (p, p): no LDS wait before 1 / pivot
      wave_sync();
      const cd bip = Ai[i * LD + p], bpj = Ai[p * LD + j];
      wave_sync();
      double inv = __builtin_amdgcn_rcp(piv);
      inv = fma(inv, fma(-piv, inv, 1.0), inv);
      inv = fma(inv, fma(-piv, inv, 1.0), inv);
      const cd t{bpj.re * inv, bpj.im * inv};
      const cd e = cmul(bip, t);
      cd nb{b.re - e.re, b.im - e.im};
      if (j == p) nb = cd{-bip.re * inv, -bip.im * inv};
      if (i == p) nb = (j == p) ? cd{inv, 0.0} : t;
      b = nb;
    };
    if constexpr (NATURAL) {
      if (!inverse) {
#pragma unroll
        for (int p = 0; p < d; ++p) eliminate(p);
      }
    } else {
#pragma unroll 1
      for (int s = inverse ? d : 0; s < d; ++s) eliminate(s < kneg ? s : (s < d - 1 ? s + 1 : kneg));
    }
    QT_STAMP(4);
    // X_k is kept at Frobenius norm 1, i.e. sum sigma_i^2 = 1; then ||X_k X_k^dagger||_F^2 = sum sigma_i^4
    // is the purity of that spectrum: one reduction per squaring gives both the scale and the test.
    b = cscale(b, fast_rsqrt(gsum<G>(b.re * b.re + b.im * b.im)));
    // At most seven squarings.  The one that certifies (defect < 1e-7) is followed by exactly one more, which ends the
    // loop with `certified` set; it ends without it behind the seventh squaring (certifying there is too late) and
    // behind the third when the ratio is slow; a helper wavefront also leaves once the trial has called the lift off
    // (it finishes the squaring it is in: the look rides on that squaring's LDS reads).  The tests are wave-uniform and
    // combined without short-circuit into ONE exit, behind which the two flags tell the ends apart: an iteration that
    // goes on pays for one branch.  (With an exit per test the compiler numbers the exits in a register and dispatches
    // on it behind the loop: about twenty scalar instructions per iteration.)
    bool certified = false, called_off = false;
#pragma unroll 1
    for (int k = 1;; ++k) {
      Ai[c.e] = b;
      wave_sync();
      [[maybe_unused]] const int verdict = c.verdict_load();  // (helper wavefront: ahead of the reads below, looked at behind them)
      cd n{0.0, 0.0}, n2{0.0, 0.0};  // even / odd terms: two dependency chains per component
#pragma unroll
      for (int q = 0; q < d; q += 2) {
        const cd u = Ai[i * LD + q], v = Ai[j * LD + q];
        n.re = fma(u.re, v.re, fma(u.im, v.im, n.re));
        n.im = fma(u.im, v.re, fma(-u.re, v.im, n.im));
        if (q + 1 < d) {
          const cd u2 = Ai[i * LD + q + 1], v2 = Ai[j * LD + q + 1];
          n2.re = fma(u2.re, v2.re, fma(u2.im, v2.im, n2.re));
          n2.im = fma(u2.im, v2.re, fma(-u2.re, v2.im, n2.im));
        }
      }
      n = cadd(n, n2);
      wave_sync();
      called_off = c.abandoned(verdict);  // helper wavefront: the trial has no use for this lift
      const double pur = gsum<G>(n.re * n.re + n.im * n.im);
      b = cscale(n, fast_rsqrt(pur));
      const double defect = 1.0 - pur;  // ~ 2 (sigma_2 / sigma_1)^(2^(k+1))
      QT_STAMP_VAL(20, k);
#ifdef QT_PHASE_TIMING
      if (k <= 5) QT_STAMP(25 + k);
#endif
      // k == 3 and not below 0.05: ratio > ~0.8, the eigensolver is cheaper (a defect below 1e-7 never takes that exit)
      if (called_off | certified | (k == 7) | ((k == 3) & !(defect < 0.05))) break;
      certified = defect < 1e-7;
    }
    QT_STAMP(5);
    if (called_off || !certified) return false;
    if (i == j) b.im = 0.0;
    b = cscale(b, 1.0 / gtrace<G>(i == j, b.re));            // N = X / Tr X
    const double lam = gsum<G>(r.re * b.re + r.im * b.im);  // Tr(A N) = sum_ij A_ij conj(N_ij)
    if constexpr (kLiftOneExit) {
      // The result needs lam and not the residual: both in one basic block, so that the trace and the divisions of
      // `out` run beside the 16-FMA chains and the two reductions of the check, and ONE wave-uniform test behind them,
      // combined without short-circuit (as in the squaring loop).  Same operations, operands and order as below.
      Ai[c.e] = r;
      Vi[c.e] = b;
      const double w = eps - lam;
      const cd o{fma(w, b.re, r.re), fma(w, b.im, r.im)};
      const double tr = gtrace<G>(i == j, o.re);
      out = cd{o.re / tr, o.im / tr};
      wave_sync();
      cd q{-lam * b.re, -lam * b.im};
#pragma unroll
      for (int k = 0; k < d; ++k) {  // (A N)_ij, N Hermitian
        const cd u = Ai[i * LD + k], v = Vi[j * LD + k];
        q.re = fma(u.re, v.re, fma(u.im, v.im, q.re));
        q.im = fma(u.im, v.re, fma(-u.re, v.im, q.im));
      }
      wave_sync();
      const double res2 = gsum<G>(q.re * q.re + q.im * q.im);
      const double nrm2 = gsum<G>(r.re * r.re + r.im * r.im);
      return (lam < eps) & (res2 <= 1e-26 * nrm2);  // (a NaN on either side refuses, as !(a < b) did)
    }
    if (!(lam < eps)) return false;
    Ai[c.e] = r;
    Vi[c.e] = b;
    wave_sync();
    cd q{-lam * b.re, -lam * b.im};
#pragma unroll
    for (int k = 0; k < d; ++k) {  // (A N)_ij, N Hermitian
      const cd u = Ai[i * LD + k], v = Vi[j * LD + k];
      q.re = fma(u.re, v.re, fma(u.im, v.im, q.re));
      q.im = fma(u.im, v.re, fma(-u.re, v.im, q.im));
    }
    wave_sync();
    const double res2 = gsum<G>(q.re * q.re + q.im * q.im);
    const double nrm2 = gsum<G>(r.re * r.re + r.im * r.im);
    if (!(res2 <= 1e-26 * nrm2)) return false;
    const double w = eps - lam;
    cd o{fma(w, b.re, r.re), fma(w, b.im, r.im)};
    const double tr = gtrace<G>(i == j, o.re);
    out = cd{o.re / tr, o.im / tr};
    return true;
  }

  // a7 with the positive-definite shortcut: when the Hermitian input is numerically positive
  // definite (its Cholesky factorisation runs through) no eigenvalue is below the clip, so
  // U max(v, 1e-15) U^dagger is the input itself (to rounding) and only the trace division is left.
  // Returns the projected element; if `xl` is non-null also the Cholesky parameter of the result.
  // C::kHelper (k_mle_fused_hw; SPEC is off there): the trial's helper wavefront, which has been lifting `r` on
  // speculation since before the sweep, is told the verdict as soon as it is known.  One negative pivot, the last: the
  // lifted matrix is the helper's, and so is its factorisation: it comes back with c.link->pending set, *xl and
  // *ok_out are not written (HelperLink::collect has them later) and *lscale_out = 1.  Every other class runs as
  // without a helper, on this wave.
  template <bool SPEC = false, class C>
  __device__ static cd make_feasible(const C& c, cd r, double* xl, int* ok_out, double* lscale_out = nullptr) {
    int ok, neg, kneg;
    cd spec_inv{0.0, 0.0};
    double x = cholesky_param<SPEC && G == 64>(c, r, ok, &neg, &kneg, &spec_inv);
    QT_STAMP(3);
    // The positive-definite epilogue: r / tr, and the Cholesky parameters of r / tr through
    // 1 / sqrt(tr): hardware seed + Newton (~1 ulp) instead of an IEEE sqrt and
    // an IEEE division (~60 instructions on the critical path); tr = 1 up to the noise of the linear inversion
    cd out{0.0, 0.0};
    double lscale = 1.0;
    auto pd_epilogue = [&]() {
      const double tr = gtrace<G>(c.i == c.j, r.re);
      out = cd{r.re / tr, r.im / tr};
      const double rst = tr > 0.0 ? fast_rsqrt(tr) : 1.0 / sqrt(tr);
      x = x * rst;   // L of r/tr
      lscale = rst;  // Bm() holds the factor of r, not of r/tr
    };
    // One trial per wave: `ok` is wave-uniform and a clipped trial replaces all of it, so it is formed only for the
    // trials that keep it.  Several trials per wave: the groups differ, every lane runs it ahead of the branch.
    const bool all_pd = __all(ok);
    [[maybe_unused]] bool go = false;
    if constexpr (C::kHelper) {
      go = kLiftSingleNegative && !all_pd && __builtin_amdgcn_readfirstlane(neg) == 1 &&
           __builtin_amdgcn_readfirstlane(kneg) == d - 1;
      c.link->decide(go);
    }
    if (G < 64 || all_pd || (!xl && lscale_out)) pd_epilogue();
    if (!all_pd) {
      cd proj;
      bool lifted = false;
      [[maybe_unused]] bool refused = false;  // by the helper: the same arithmetic on this wave would refuse again
      if constexpr (C::kHelper) {
        if (go) {
          const int came = c.link->await_lift(c.e, proj);
          QT_STAMP(31);
          if (came == HelperLink::kLifted) {
            QT_STAMP(6);
            if (lscale_out) *lscale_out = 1.0;
            return proj;
          }
          refused = came == HelperLink::kRefused;
        }
      }
      if constexpr (G == 64) {  // one trial per wave: neg / kneg are the same in every lane
        if (kLiftSingleNegative && !refused && __builtin_amdgcn_readfirstlane(neg) == 1) {
          const int kn = __builtin_amdgcn_readfirstlane(kneg);
          lifted = __builtin_amdgcn_readfirstlane(
                       (int)lift_single_negative(c, r, kn, 1e-15, proj, SPEC && kn == d - 1 ? &spec_inv : nullptr)) != 0;
        }
      }
      if (!lifted) proj = psd_project(c, r, 1e-15);  // whole wave runs it; PD trials keep their shortcut
      QT_STAMP(6);
      int ok2 = 1;
      double x2 = xl ? cholesky_param(c, proj, ok2) : 0.0;
      if (lifted && xl && !__all(ok2 || ok)) {
        // the short cut left something non-positive behind (an inertia count thrown off by a pivot at
        // rounding level): take the eigensolver after all
        proj = psd_project(c, r, 1e-15);
        x2 = cholesky_param(c, proj, ok2);
      }
      QT_STAMP(7);
      if (xl) lscale = 1.0;  // the whole wave went through the second factorisation: Bm() = factor of proj
      if (!ok) {
        out = proj;
        x = x2;
        ok = ok2;
      }
    }
    if (xl) *xl = x;
    if (ok_out) *ok_out = ok;
    if (lscale_out) *lscale_out = lscale;
    return out;
  }

  // x (one parameter per lane) -> L in Bm(), returns lane's element of L L^dagger and t = Tr.
  template <class C>
  __device__ static cd build_llh(const C& c, double xl, double& tr) {
    double* vx = c.vec();
    cd* L = c.Bm();
    vx[c.l] = xl;
    tr = gsum<G>(xl * xl);
    wave_sync();
    const int i = c.i, j = c.j;
    L[c.e] = cd{vx[c.src_re], vx[c.src_im]};  // branch-free: the zero slot feeds the upper triangle
    wave_sync();
    cd m{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) {  // all k: the zeros of L contribute exact zeros
      const cd u = L[i * LD + k], v = L[j * LD + k];
      m.re = fma(u.re, v.re, fma(u.im, v.im, m.re));
      m.im = fma(u.im, v.re, fma(-u.re, v.im, m.im));
    }
    return m;
  }

  // ---- a9: NLL value and exact gradient at x (operand Aw).  Needs freq[] loaded.  Leaves L in Bm().
  // `start` (first evaluation of a trial, at the Cholesky parameters of a matrix that is still at hand):
  // rho(x) = L L^dagger / Tr is that matrix, and its factor already sits in Bm() up to the scale
  // start->lscale, so L L^dagger is not formed again.
  struct StartPoint {
    cd rho;         // this lane's element of the normalised start matrix
    double lscale;  // L(x) = lscale * Bm()
  };
  // DEFER (specialised kernels only): `f` is left alone; `dv` receives what deferred_value needs to form it later.
  // LATE (with `start`; k_mle_fused_hw): the parameters are not known yet.  Everything up to the gradient matrix reads
  // only start->rho; x is first needed for Tr = sum x^2 behind it, and the trial's helper wavefront has it by then
  // (HelperLink::collect, LateX).
  template <bool DEFER = false, class C, bool LATE = false>
  __device__ static void nll_grad(const C& c, double xl, double& f, double& gl, cd* rho_l = nullptr,
                                  bool want_grad = true, const StartPoint* start = nullptr, DeferredValue* dv = nullptr) {
    static_assert(!DEFER || !C::kGeneric, "the deferred value needs the compile-time row count of the specialised shape");
    double tr;
    QT_STAMP(11);
    cd m;
    if constexpr (LATE) {
      m = start->rho;  // (not read: rho_e below is start->rho)
    } else if (start) {
      tr = gsum<G>(xl * xl);
      m = cd{start->rho.re * tr, start->rho.im * tr};
    } else {
      m = build_llh(c, xl, tr);
    }
    QT_STAMP(12);
    cd* A = c.A();
    const cd rho_e = start ? start->rho : cd{m.re / tr, m.im / tr};
    if (rho_l) *rho_l = rho_e;
    A[c.e] = rho_e;
    wave_sync();
    const double bl = bloch_of(c, A);
    QT_STAMP(13);
    double* vec = c.vec();
    // (n = 3 with lane tables: bloch_of has just left the whole Bloch vector in vec and read this element back from
    // it -- a second store of it would only put an LDS round trip in front of the first forward stage)
    if constexpr (!(NQ == 3 && C::kLaneTables != 0 && kLaneLeftovers)) {
      vec[c.l] = bl;
      wave_sync();
    }
    // p = d * A' b ;  f = -sum freq log(p + 1e-10) ;  r = freq / (p + 1e-10)
    double fpart = 0.0;
    const double* fr = c.freq();
    double* rb = c.rbuf();
    double wl;
    if (c.prod()) {
      const int R1 = c.R1();
      const bool paired = c.pairedT() != 0;
      const int* tab = c.tfwd;
      const double* in = vec;
#pragma unroll
      for (int q = 1; q < NQ; ++q) {  // stages 1 .. n-1; the last of them lands in bufB
        const int stride = 1 << (2 * (NQ - q));
        const int n_out = ipow(R1, q) * stride;
        double* out = ((NQ - 1 - q) & 1) ? rb : c.bufB();
        if (paired) {
          paired_forward(c, q, in, out);
        } else if constexpr (C::kGeneric) {
          stage<true>(c, c.tabT(), tab, n_out, stride, in, out);
          tab += n_out;
        }
        in = out;
      }
      QT_STAMP(14);
      if constexpr (DEFER) {
        stage_n_log<true, true, true>(c, tab, in, fr, rb, dv);
      } else if constexpr (!C::kGeneric) {
        fpart = stage_n_log<true, true>(c, tab, in, fr, rb);
      } else {
        if (!paired) fpart = stage_n_log<false, false>(c, tab, in, fr, rb);
        else if (c.uniform()) fpart = stage_n_log<true, true>(c, tab, in, fr, rb);
        else fpart = stage_n_log<true, false>(c, tab, in, fr, rb);
      }
      if constexpr (!DEFER) f = -gsum<G>(fpart);
      wave_sync();
      QT_STAMP(15);
      if (!want_grad) return;  // (uniform) the Metropolis chain only needs the value
      wl = prod_backward<false>(c, rb);
      QT_STAMP(16);
    } else if constexpr (C::kGeneric) {
      for (int m0 = 0; m0 < c.M; m0 += G) {
        const int mm = m0 + c.l;
        if (mm < c.M) {
          const double pe = row_dot(c, c.pv.AwT, mm, vec) * d + 1e-10;
          fpart += fr[mm] * fast_log(pe);
          rb[mm] = fr[mm] * recip_nr(pe);
        }
      }
      f = -gsum<G>(fpart);
      wave_sync();
      if (!want_grad) return;
      // w = A'^T r ;  G = -sum_k w_k P_k ;  Gt = (G - Tr(G rho) I) / t
      wl = col_dot(c, c.pv.Aw, rb);
    }
    const double tr_g_rho = -(double)d * gsum<G>(wl * bl);
    vec[c.l] = wl;
    wave_sync();
    cd g = matrix_of(c, vec);
    QT_STAMP(17);
    // (LATE: collect in front of matrix_of, so that the poll, Tr and the divisions' denominator half overlap its add
    // chain, was measured 0.07 us SLOWER: profiles/lift_tail_headline_ab.txt)
    if constexpr (LATE) {
      LateX& lx = *c.late;
      lx.x = 1.0;
      lx.ok = 0;
      lx.got = c.link->collect(c.l, lx.x, lx.ok);
      xl = lx.x;
      tr = gsum<G>(xl * xl);
      QT_STAMP(25);
    }
    g.re = -g.re;
    g.im = -g.im;
    if (c.i == c.j) g.re -= tr_g_rho;
    g.re /= tr;
    g.im /= tr;
    A[c.e] = g;
    wave_sync();
    // Q = Gt L ; gradient entries 2 Re Q_ii, 2 Re Q_ij, 2 Im Q_ij (i > j)
    const cd* L = c.Bm();
    cd q{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < d; ++k) {  // all k: L[k][pj] = 0 above the diagonal
      const cd u = A[c.pi * LD + k], v = L[k * LD + c.pj];
      q.re = fma(u.re, v.re, fma(-u.im, v.im, q.re));
      q.im = fma(u.re, v.im, fma(u.im, v.re, q.im));
    }
    gl = 2.0 * (c.pkind == 2 ? q.im : q.re);
    if (start) gl *= start->lscale;
    wave_sync();
    QT_STAMP(18);
  }

  // sqrt(|Tr((R - C)^2)|) / sqrt(2) for the matrix R held one element (i, j) per lane (geometry.py:16-20):
  // Tr(Delta Delta) = sum_ij Delta_ij Delta_ji, the transposed element fetched from lane (j, i) of the group.
  // Executed by every lane of the wavefront (DPP reductions); every lane of a group returns the same bits.
  template <class C>
  __device__ __forceinline__ static double hs_to_centre(const C& c, cd r, const double* __restrict__ centre) {
    const double2 cc = *reinterpret_cast<const double2*>(centre + 2 * c.l);
    const cd dl{r.re - cc.x, r.im - cc.y};
    const int src = (int)(threadIdx.x & 63) - c.l + c.j * d + c.i;
    const cd dt{__shfl(dl.re, src, 64), __shfl(dl.im, src, 64)};
    const cd t = hs_term(dl, dt);
    const double sr = gsum<G>(t.re);
    const double si = gsum<G>(t.im);
    const double v = sqrt(hypot(sr, si)) / sqrt(2.0);
    return v < 1e-15 ? 0.0 : v;
  }
  // Result of trial b: element (i, j) = r.  `store` = this lane's group owns a live trial; the distance is computed by
  // all lanes (o.dist is uniform over the launch), only the stores are masked.
  template <class C>
  __device__ __forceinline__ static void emit(const C& c, const EstOut& o, int b, bool store, cd r) {
    if (o.dist) {
      const double v = hs_to_centre(c, r, o.centre_of(b, 2 * D));  // b: this lane group's trial
      if (store && c.l == 0) o.dist[b] = v;
    }
    if (store && o.rho) {
      double* out = o.rho + ((size_t)b * D + c.l) * 2;
      out[0] = r.re;
      out[1] = r.im;
    }
  }
  // The two halves of emit on their own: mle_fused_body stores the matrix in front of the first evaluation and the
  // distance behind it.
  template <class C>
  __device__ __forceinline__ static void emit_dist(const C& c, const EstOut& o, int b, bool store, cd r) {
    if (o.dist) {
      const double v = hs_to_centre(c, r, o.centre_of(b, 2 * D));
      if (store && c.l == 0) o.dist[b] = v;
    }
  }
  template <class C>
  __device__ __forceinline__ static void emit_rho(const C& c, const EstOut& o, int b, bool store, cd r) {
    if (store && o.rho) {
      double* out = o.rho + ((size_t)b * D + c.l) * 2;
      out[0] = r.re;
      out[1] = r.im;
    }
  }
};

// =========================================================================================
// kernels (workgroup = 4 waves; a wave owns 64/G trials; `live` masks the padding of the last block)
// =========================================================================================

// a6 + a7
template <int NQ>
__global__ void __launch_bounds__(256) k_lin_batch(PovmView pv, const int64_t* __restrict__ counts, int B, int physical,
                                                   EstOut rho, double* __restrict__ bloch_out,
                                                   int32_t* __restrict__ status) {
  using S = Small<NQ>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;  // padding groups recompute the last trial; nothing is stored
  typename S::Prefetch pf;
  S::prefetch_counts(pf, counts + (size_t)bb * pv.M, pv);
  S::make_ctx(c, smem, pv);
  QT_STAMP(0);
  const bool shots_ok = S::load_freq(c, counts + (size_t)bb * pv.M, &pf);
  QT_STAMP(1);
  double bl;
  cd r = S::lin_invert(c, bl);
  QT_STAMP(2);
  if (physical) r = S::make_feasible(c, r, nullptr, nullptr);
  QT_STAMP(9);
  S::emit(c, rho, b, live, r);
  if (live) {
    if (bloch_out) bloch_out[(size_t)b * S::D + c.l] = bl;
    if (status && c.l == 0) status[b] = !shots_ok ? 5 : (r.re == r.re) ? 0 : 4;
  }
}

// a8 forward: rho -> x
template <int NQ>
__global__ void __launch_bounds__(256) k_chol_param(PovmView pv, const double* __restrict__ rho, int B,
                                                    double* __restrict__ x, int32_t* __restrict__ status) {
  using S = Small<NQ>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  S::make_ctx(c, smem, pv);
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;
  const double* in = rho + ((size_t)bb * S::D + c.l) * 2;
  int ok;
  const double xl = S::cholesky_param(c, cd{in[0], in[1]}, ok);
  if (live) {
    x[(size_t)b * S::D + c.l] = xl;
    if (status && c.l == 0) status[b] = ok ? 0 : 1;
  }
}

// a8 backward: x -> L L^dagger
template <int NQ>
__global__ void __launch_bounds__(256) k_chol_unparam(PovmView pv, const double* __restrict__ x, int B,
                                                      double* __restrict__ llh) {
  using S = Small<NQ>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  S::make_ctx(c, smem, pv);
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;
  double tr;
  const cd m = S::build_llh(c, x[(size_t)bb * S::D + c.l], tr);
  if (live) {
    double* out = llh + ((size_t)b * S::D + c.l) * 2;
    out[0] = m.re;
    out[1] = m.im;
  }
}

// Trace distance / infidelity of a batch to a table of centres (geometry.py:23-56; Small::trace_dist, Small::infidelity).
enum Metric { kMetricTrace = 0, kMetricInfidelity = 1 };

// roots[g] = the Hermitian root of centres[g] (Small::psd_sqrt), g < G: the set-up launch of the infidelity, once per call
template <int NQ>
__global__ void __launch_bounds__(256) k_psd_sqrt(const double* __restrict__ centres, int G, double jtol2,
                                                  double* __restrict__ roots) {
  using S = Small<NQ>;
  __shared__ __attribute__((aligned(16))) double smem[S::TPB * S::kMetricDoubles];
  typename S::CtxM c;
  S::make_ctx_metric(c, smem, jtol2);
  bool live;
  const int g = S::trial_index(G, &live);
  const int gg = live ? g : G - 1;
  const double* in = centres + ((size_t)gg * S::D + c.l) * 2;
  const cd s = S::psd_sqrt(c, cd{in[0], in[1]});
  if (live) {
    double* out = roots + ((size_t)g * S::D + c.l) * 2;
    out[0] = s.re;
    out[1] = s.im;
  }
}

// dist[b] = METRIC(rho[b], centre (g0 + b) % G).  `centres`: the centres themselves (trace distance) or their roots as
// k_psd_sqrt left them (infidelity).  A trial's bits depend on its two matrices alone: not on B, its place in the batch,
// its wavefront neighbours (jacobi_sweeps<OWN>) or G.
template <int NQ, int METRIC>
__global__ void __launch_bounds__(256) k_metric_dist(const double* __restrict__ rho, int B,
                                                     const double* __restrict__ centres, int G, int g0, double jtol2,
                                                     double* __restrict__ dist) {
  using S = Small<NQ>;
  __shared__ __attribute__((aligned(16))) double smem[S::TPB * S::kMetricDoubles];
  typename S::CtxM c;
  S::make_ctx_metric(c, smem, jtol2);
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;  // padding groups recompute the last trial; nothing is stored
  const double* in = rho + ((size_t)bb * S::D + c.l) * 2;
  const double* cen = centre_of(centres, G, g0, bb, 2 * S::D) + 2 * c.l;
  const cd r{in[0], in[1]}, q{cen[0], cen[1]};
  const double v = METRIC == kMetricTrace ? S::trace_dist(c, r, q) : S::infidelity(c, r, q);
  if (live && c.l == 0) dist[b] = v;
}

// a9
template <int NQ>
__global__ void __launch_bounds__(256) k_nll_batch(PovmView pv, const double* __restrict__ x,
                                                   const int64_t* __restrict__ counts, int B, double* __restrict__ f,
                                                   double* __restrict__ grad) {
  using S = Small<NQ>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  S::make_ctx(c, smem, pv);
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;
  S::load_freq(c, counts + (size_t)bb * pv.M);
  double fv, gl;
  S::nll_grad(c, x[(size_t)bb * S::D + c.l], fv, gl);
  if (live) {
    if (c.l == 0) f[b] = fv;
    if (grad) grad[(size_t)b * S::D + c.l] = gl;
  }
}

}  // namespace qt
