// Wave-level primitives shared by every kernel family: the phase stamps (QT_STAMP), the complex element `cd`, the
// LDS hand-off inside a wavefront (wave_sync), the DPP reductions over a lane group (gsum, gtrace, gmax, group_any), the
// short log / reciprocal / rsqrt, the streamed dot product (dot_global) and the Jacobi rotation.  Depends on nothing
// else of the project's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qt {

// Optional per-wave phase stamps (shader clock) for scripts/phase_timing.py: compiled in only with
// -DQT_PHASE_TIMING (lib/libqtomo_prof.so); the product library carries none of this.
#ifdef QT_PHASE_TIMING
__device__ long long* g_qt_prof = nullptr;  // [waves][32]
// One row per wavefront of threadIdx.y = 0; the helper wavefronts of k_mle_fused_hw (threadIdx.y = 1) have theirs behind
// those of the whole grid, in the same order.
#define QT_PROF_ROW \
  ((size_t)(blockIdx.x + threadIdx.y * gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6))
#define QT_STAMP(slot)                                                                                   \
  do {                                                                                                   \
    if (g_qt_prof && (threadIdx.x & 63) == 0)                                                            \
      g_qt_prof[QT_PROF_ROW * 32 + (slot)] = (long long)__builtin_readcyclecounter();                    \
  } while (0)
#define QT_STAMP_VAL(slot, val)                                                                          \
  do {                                                                                                   \
    if (g_qt_prof && (threadIdx.x & 63) == 0)                                                            \
      g_qt_prof[QT_PROF_ROW * 32 + (slot)] = (val);                                                      \
  } while (0)
#else
#define QT_STAMP(slot) do {} while (0)
#define QT_STAMP_VAL(slot, val) do {} while (0)
#endif

// 16-byte aligned: a complex element then moves with ONE ds_read_b128 / ds_write_b128 (4 LDS cycles per
// wavefront read, conflict-free on consecutive elements).  With 8-byte alignment hipcc emits ds_read2_b64 /
// ds_write2_b64, whose two 8-byte halves each stride 16 bytes across the lanes: a built-in 2-way bank
// conflict, 16 cycles per read (measured on the n = 5 Jacobi rounds: 2700 -> see DESIGN 4.5).  Every cd
// array in LDS starts at an even double offset (checked where the layouts are defined).
struct alignas(16) cd {
  double re, im;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cd cmulc(cd a, cd b) {  // a * conj(b)
  return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}
__device__ __forceinline__ cd cadd(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
// One term Delta_ij Delta_ji of Tr(Delta^2) (geometry.py:16), with its rounding pinned (one product rounded, then one
// fma) so that every kernel that forms a Hilbert-Schmidt distance gets the same bits from the same operands.
__device__ __forceinline__ cd hs_term(cd a, cd b) {
  return {__builtin_fma(a.re, b.re, -(a.im * b.im)), __builtin_fma(a.re, b.im, a.im * b.re)};
}
__device__ __forceinline__ cd cscale(cd a, double s) { return {a.re * s, a.im * s}; }

// LDS hand-off inside ONE wavefront: order this wave's LDS writes before its later reads.  The hardware already does:
// the LDS executes the DS instructions of a wavefront in issue order, each for all 64 lanes before the next starts, so a
// ds_read behind a ds_write of the same wave sees the data whichever lane wrote it.  What is needed is that the
// COMPILER keeps the order (to it, another lane's slot is just a different address): a scheduling barrier plus an
// empty asm with a memory clobber.  Rounds 1-2 used release / acquire fences at workgroup scope here, which cost an
// `s_waitcnt lgkmcnt(0)` -- a full drain of the LDS queue, ~100 clocks -- at each of the ~100 hand-offs of a trial.
// (Never a cross-wave hand-off: every use is inside one trial's own scratch; tables shared by a workgroup are
// published by __syncthreads.)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

// ---- group reductions on the DPP network (no LDS round trips) ---------------------------------
// A butterfly inside rows of 16 lanes (quad_perm, row_half_mirror, row_mirror) and, for G = 64,
// four v_readlane across the rows.  Every lane of a group ends with the same bits.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_f64(double v) {
  // Full row mask and bound_ctrl: a lane without a source reads 0 and the compiler needs no zero-initialisation of the
  // destination.  Under the permutations inside a row every lane has a source.  The row_bcast steps once ran with a
  // partial row mask (0xA, 0xC) so that the rows they do not feed kept their values, which took an initialised
  // destination (two v_mov_b32 v, 0 per step).  Nothing needs that: the reductions hand out lane 63 alone, whose tree
  // (r3 + r2) + (r1 + r0) reads lane 47 in the first step and lane 31 -- row 1, fed by the first step -- in the second.
  // With the full mask rows 0 (first step) and 0 - 1 (second) add a 0 to values that nobody reads.  ROW_MASK stays a
  // parameter for a caller that does read the other rows.
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffLL), CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, ROW_MASK == 0xf);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffLL), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double nanmax(double a, double b) { return (b > a || b != b) ? b : a; }  // NaN wins

// Across the four rows of a wavefront: row_bcast15 adds the total of row 0 / 2 into row 1 / 3,
// row_bcast31 adds lane 31 (rows 0+1) into rows 2 and 3, lane 63 then holds (r2 + r3) + (r0 + r1) and
// is handed to every lane through an SGPR pair (6 + 2 instructions instead of 8 readlanes + 7).  Lane 63 is the only
// lane anybody reads: what the two steps leave in rows 0 - 2 is not a sum of anything (see dpp_f64).
template <int G>
__device__ __forceinline__ double gsum(double v) {
  v += dpp_f64<0xB1>(v);                 // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);                 // quad_perm [2,3,0,1]
  if (G >= 8) v += dpp_f64<0x141>(v);    // row_half_mirror
  if (G >= 16) v += dpp_f64<0x140>(v);   // row_mirror
  if (G == 64) {
    v += dpp_f64<0x142>(v);              // row_bcast15: lane 15 of row 0 / 1 / 2 -> rows 1 / 2 / 3 (row 0: + 0)
    v += dpp_f64<0x143>(v);              // row_bcast31: lane 31 -> rows 2, 3 (rows 0, 1: + 0)
    v = readlane_f64(v, 63);
  }
  return v;
}
// Trace of a d x d matrix held one element per lane (lane = i d + j): the bits of gsum<G>(diag ? x : 0.0), `diag` = this
// lane is (i, i).  At G = 64 (d = 8) the diagonal sits in lanes 9 i, two per row at positions 2 r and 2 r + 9 of row r,
// in different halves of the row: in gsum's butterfly the first three steps add + 0.0 to each of them three times and
// the two of a row first meet in row_mirror, where lane 15 forms x(2 r + 9) + x(2 r).  Here one + 0.0 stands for the
// three (x + 0.0 is x except that it turns -0.0 into +0.0, and it is idempotent: without it a diagonal of nothing but
// -0.0 would give -0.0 where gsum gives +0.0), row_shr:9 forms the same sum, same operand order, in lane 2 r + 9 of
// each row, and as those lanes are not the lane 15 that row_bcast reads, the three sums across the rows go through
// SGPR pairs: (s3 + s2) in lane 63, (s1 + s0) in lane 27, then their sum in lane 63 -- gsum's tree.  17 instructions
// as compiled for the 28 of gsum<64> with the select in front of it (profiles/chain_diet_isa.txt).
template <int G>
__device__ __forceinline__ double gtrace(bool diag, double x) {
  double v = diag ? x : 0.0;
  if (G != 64) return gsum<G>(v);
  v += 0.0;
  v += dpp_f64<0x119>(v);                              // row_shr:9, lanes 0 - 8 of a row read 0: s_r in lane 18 r + 9
  const double hi = v + readlane_f64(v, 45);           // lane 63: s3 + s2
  const double lo = v + readlane_f64(v, 9);            // lane 27: s1 + s0
  return readlane_f64(hi + readlane_f64(lo, 27), 63);  // lane 63: (s3 + s2) + (s1 + s0)
}
// "Does `pred` hold in any lane of this lane's group": one ballot and a mask (the whole wave at G = 64).  Executed by
// every lane of the wavefront.
template <int G>
__device__ __forceinline__ bool group_any(bool pred) {
  const unsigned long long votes = __builtin_amdgcn_ballot_w64(pred);
  if (G == 64) return votes != 0ull;
  const int lane = threadIdx.x & 63;
  return (votes & (((1ull << (G & 63)) - 1ull) << (lane / G * G))) != 0ull;
}
// v_max_f64 as it stands: of a NaN and a number it returns the number.  (fmax() in C++ makes the compiler put a
// canonicalising v_max_f64 v, v, v in front of the operand that comes out of a DPP move -- one extra instruction per
// level of the butterfly below: 49 instead of 42 for gmax<64>, against 63 for the compare-and-select form.)
__device__ __forceinline__ double max_f64(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// Maximum of non-negative values (every caller passes fabs(.)); a NaN anywhere wins: the butterfly itself passes over
// NaNs, one ballot finds them.  The rows a row_bcast step does not feed take the maximum with 0: neutral for such inputs,
// and none of them is on the way to lane 63.
template <int G>
__device__ __forceinline__ double gmax(double v) {
  const bool nan = group_any<G>(v != v);
  v = max_f64(v, dpp_f64<0xB1>(v));
  v = max_f64(v, dpp_f64<0x4E>(v));
  if (G >= 8) v = max_f64(v, dpp_f64<0x141>(v));
  if (G >= 16) v = max_f64(v, dpp_f64<0x140>(v));
  if (G == 64) {
    v = max_f64(v, dpp_f64<0x142>(v));
    v = max_f64(v, dpp_f64<0x143>(v));
    v = readlane_f64(v, 63);
  }
  return nan ? __builtin_nan("") : v;
}

// log(x) and 1/x for the likelihood terms.  The OCML log is correctly rounded through ~85 FP64
// instructions of double-double arithmetic; the NLL needs neither that nor the special cases beyond
// "x <= 0 or NaN gives NaN / -inf", and a lone wave pays for every instruction.  x = m 2^e with
// m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1), log m = 2 s (1 + s^2/3 + s^4/5 + ...): with
// s^2 <= 0.0295 ten terms reach 2^-55; error ~1.5 ulp.  About 30 instructions.
__device__ __forceinline__ double recip_nr(double x) {  // 1/x to ~1 ulp: hardware seed + two Newton steps
  double r = __builtin_amdgcn_rcp(x);
  r = fma(r, fma(-x, r, 1.0), r);
  return fma(r, fma(-x, r, 1.0), r);
}
__device__ __forceinline__ bool log_is_regular(double x) { return x > 0.0 && x < 1.7e308; }  // fast_log's main branch
__device__ __forceinline__ double fast_log(double x) {
  if (!(x > 0.0) || !(x < 1.7e308)) return x == 0.0 ? -__builtin_huge_val() : (x > 0.0 ? x : __builtin_nan(""));
  double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? m + m : m;
  e = low ? e - 1 : e;
  const double num = m - 1.0, den = m + 1.0;
  const double r = recip_nr(den);
  double sq = num * r;
  sq = fma(r, fma(-sq, den, num), sq);  // s = num / den, correctly rounded up to the last bit
  const double z = sq * sq;
  // P(z) = 1/3 + z/5 + ... + z^9/21, Estrin's scheme: pairs, then powers z^2, z^4, z^8 (dependency depth 5
  // instead of the 10 of Horner's rule)
  const double z2 = z * z, z4 = z2 * z2, z8 = z4 * z4;
  const double q0 = fma(z, 1.0 / 5.0, 1.0 / 3.0), q1 = fma(z, 1.0 / 9.0, 1.0 / 7.0);
  const double q2 = fma(z, 1.0 / 13.0, 1.0 / 11.0), q3 = fma(z, 1.0 / 17.0, 1.0 / 15.0);
  const double q4 = fma(z, 1.0 / 21.0, 1.0 / 19.0);
  const double r0 = fma(z2, q1, q0), r1 = fma(z2, q3, q2);
  const double pl = fma(z8, q4, fma(z4, r1, r0));
  const double lm = fma(sq + sq, pl * z, sq + sq);  // 2 s (1 + z P(z))
  const double ed = (double)e;
  return fma(ed, 6.93147180369123816490e-01, fma(ed, 1.90821492927058770002e-10, lm));  // e ln2 (hi + lo) + log m
}

// 1/sqrt(x) for normal-range positive x: hardware seed (v_rsq_f64) plus two Newton steps -- ~8
// dependent FP64 instructions instead of the ~25 of a correctly rounded sqrt-then-divide,
// accurate to ~1 ulp, which is all a Jacobi rotation / Cholesky pivot needs.
__device__ __forceinline__ double fast_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  double e = fma(-x * y, y, 1.0);
  y = fma(y * e, fma(e, 0.375, 0.5), y);
  e = fma(-x * y, y, 1.0);
  return fma(y * e, 0.5, y);
}

// sum_m base[m * stride + lane_off] * lds_vec[m], m < n, operand streamed from global memory (L2):
// the loads of a block of UNR rows are issued back to back before any is consumed (the
// sched_group_barriers pin that order; hipcc otherwise interleaves load / wait / FMA pairs), and
// four accumulators keep the FP64 FMAs from forming a single dependency chain.
template <int UNR>
__device__ __forceinline__ void dot_block(const double* __restrict__ base, size_t stride, unsigned lane_off,
                                          const double* lds_vec, int m, double (&acc)[4]) {
  double av[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) av[u] = base[(size_t)(m + u) * stride + lane_off];
#pragma unroll
  for (int u = 0; u < UNR; ++u) acc[u & 3] = fma(av[u], lds_vec[m + u], acc[u & 3]);
  __builtin_amdgcn_sched_group_barrier(0x020, UNR, 0);
#pragma unroll
  for (int u = 0; u < UNR; u += 4) {
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
  }
}
template <int UNR>
__device__ __forceinline__ double dot_global(const double* __restrict__ base, size_t stride, unsigned lane_off,
                                             const double* lds_vec, int n) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int m = 0;
  for (; m + UNR <= n; m += UNR) dot_block<UNR>(base, stride, lane_off, lds_vec, m, acc);
  if (UNR > 8 && m + 8 <= n) {
    dot_block<8>(base, stride, lane_off, lds_vec, m, acc);
    m += 8;
  }
  if (UNR > 4 && m + 4 <= n) {
    dot_block<4>(base, stride, lane_off, lds_vec, m, acc);
    m += 4;
  }
  for (; m < n; ++m) acc[0] = fma(base[(size_t)m * stride + lane_off], lds_vec[m], acc[0]);
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// Unitary 2x2 rotation J = [[c, w], [-conj(w), c]] that (nearly) annihilates a_pq of
// [[app, apq], [conj(apq), aqq]]: with delta = (aqq - app)/2 and
// u = t/|apq| = sign(delta) / (|delta| + sqrt(delta^2 + |apq|^2)):  c = 1/sqrt(1 + u^2 |apq|^2),
// w = s e^{i phi} = c u apq.  Only c has to be accurate (it makes J unitary for whatever u is
// used); u comes from hardware seeds with one Newton step each (~1e-13): the rotated a_pq is
// kept as computed instead of being set to zero, so an inexact angle costs convergence speed
// (nothing measurable), never accuracy.
__device__ __forceinline__ void rotation(double app, double aqq, cd apq, double& cs, cd& w) {
  const double ab2 = apq.re * apq.re + apq.im * apq.im;
  cs = 1.0;
  w = cd{0.0, 0.0};
  if (ab2 > 1e-300) {
    const double dl = 0.5 * (aqq - app);
    const double x = fma(dl, dl, ab2);
    double y = __builtin_amdgcn_rsq(x);
    y = fma(y * fma(-x * y, y, 1.0), 0.5, y);
    const double den = fabs(dl) + x * y;  // |delta| + sqrt(delta^2 + |apq|^2)
    double z = __builtin_amdgcn_rcp(den);
    z = fma(z, fma(-den, z, 1.0), z);
    const double u = copysign(z, dl);
    cs = fast_rsqrt(fma(u * u, ab2, 1.0));
    const double cu = cs * u;
    w = cd{cu * apq.re, cu * apq.im};
  }
}

}  // namespace qt
