// The 'states' process estimator (reference process.py:316-327) behind qt_states_choi_batch and its siblings: the Choi
// matrix of a trial from its D = 4^n reconstructed output states, the device form of Channel.is_cptp, and the small
// kernels that compact the failing trials for the Dykstra projection (qtomo.hip: project) and put its results back.
//
// Assembly.  With the host-built weights W[(i,j)][s] = sum_e unit_e[i][j] c_e,s the reference's sum over single-entry
// matrices is one D x D by D x D complex product per trial and a permutation of the result's index:
//     C_b[(i,k)][(j,l)] = sum_s W[(i,j)][s] rho_b,s[k][l].
// Every size takes the same mapping, 4 D threads per trial: thread u holds the column q = (k,l) = u % D of the product
// and the D / 4 rows p = (i,j) = (u / D) * (D / 4) + e.  That is 16 lanes per trial at n = 1 (four trials per wavefront,
// sixteen per workgroup), one wavefront per trial at n = 2 and one workgroup per trial at n = 3.  A trial's states are
// staged in LDS ([s][q]: consecutive lanes read consecutive elements); W is read through L1 / L2 -- a row's D elements
// are contiguous and the same for a quarter of the trial's threads (for a whole wavefront at n = 3).  Every output is
// one chain over s = 0 .. D - 1 in that order, whatever the batch: a trial's bits depend on its own inputs only.
//
// CPTP test.  ok[b] = 1 when C_b would pass Channel.is_cptp(atol):
//   * no entry of C_b is non-finite;
//   * trace preservation: R[i][j] = sum_k C[(i,k)][(j,k)] has |R - 1| <= atol + 1e-5 |1| element by element on the complex
//     modulus (np.allclose's rule: rtol at its default 1e-5, so the diagonal gets 1e-5 more than the off-diagonal);
//   * complete positivity: Herm(C) + atol 1 has an L D L^H factorisation with positive pivots, that is, the smallest
//     eigenvalue of the Hermitian part of C is >= -atol.
// The factorisation is right-looking on an LDS image of pitch D + 1 (a column read is then conflict-free), one barrier
// per column, with the same 4 D threads per trial; it never leaves early, so every thread reaches every barrier.
// CONTRACT: the flag equals the host's is_cptp whenever the smallest eigenvalue and the largest trace-preservation
// residual are both farther than 1e-9 from their thresholds; inside that band either answer is allowed.  (A completed
// factorisation is that of a matrix within ~D^2 eps |C| ~ 1e-12 of the one given, so a first non-positive pivot and a
// negative eigenvalue can disagree only that close to the threshold.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_wave.h"  // cd

namespace qt {

template <int DC>
struct StatesChoi {
  static_assert(DC == 2 || DC == 4 || DC == 8, "n = 1, 2, 3");
  static constexpr int d = DC, D = DC * DC;
  static constexpr int NT = 256;
  static constexpr int TT = 4 * D;     // threads per trial
  static constexpr int TPB = NT / TT;  // trials per workgroup: 16, 4, 1
  static constexpr int ROWS = D / 4;   // rows of the product per thread
  static constexpr int LD = D + 1;     // row pitch of the test's image
  static constexpr size_t kAssemblyLds = (size_t)TPB * D * D * sizeof(cd);     // 4, 16, 64 KB
  static constexpr size_t kTestLds = (size_t)TPB * (D * LD + 1) * sizeof(cd);  // the images and a flag slot per trial
};

// states [B][D][d][d] complex, weights [D][D] complex (row (i,j) = i d + j, column s), choi [B][D][D] complex
template <int DC>
__global__ void __launch_bounds__(256) k_states_choi(const double* __restrict__ states, int B, const double* __restrict__ weights,
                                                     double* __restrict__ choi) {
  using W = StatesChoi<DC>;
  constexpr int d = W::d, D = W::D;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x, slot = t / W::TT, u = t % W::TT;
  const int b = blockIdx.x * W::TPB + slot;
  const bool live = b < B;
  cd* rho = reinterpret_cast<cd*>(smem) + (size_t)slot * D * D;
  if (live) {
    const cd* src = reinterpret_cast<const cd*>(states) + (size_t)b * D * D;
    for (int e = u; e < D * D; e += W::TT) rho[e] = src[e];
  }
  __syncthreads();
  if (!live) return;  // (no barrier below)
  const int q = u % D;
  int p0 = (u / D) * W::ROWS;
  if (DC == 8) p0 = __builtin_amdgcn_readfirstlane(p0);  // one quarter per wavefront: the rows of W are wave-uniform
  const cd* w = reinterpret_cast<const cd*>(weights) + (size_t)p0 * D;
  cd acc[W::ROWS];
#pragma unroll
  for (int e = 0; e < W::ROWS; ++e) acc[e] = cd{0.0, 0.0};
  for (int s = 0; s < D; ++s) {
    const cd r = rho[s * D + q];
#pragma unroll
    for (int e = 0; e < W::ROWS; ++e) {
      const cd a = w[e * D + s];
      acc[e].re = __builtin_fma(a.re, r.re, acc[e].re);
      acc[e].re = __builtin_fma(-a.im, r.im, acc[e].re);
      acc[e].im = __builtin_fma(a.re, r.im, acc[e].im);
      acc[e].im = __builtin_fma(a.im, r.re, acc[e].im);
    }
  }
  cd* out = reinterpret_cast<cd*>(choi) + (size_t)b * D * D;
  const int k = q / d, l = q % d;
#pragma unroll
  for (int e = 0; e < W::ROWS; ++e) {
    const int p = p0 + e, i = p / d, j = p % d;
    out[(i * d + k) * D + j * d + l] = acc[e];
  }
}

// choi [B][D][D] complex -> ok [B] (1: passes is_cptp(atol), 0: fails).  See the head of this file.
// `failing` (nullable) [B + 1]: failing[b] = 1 - ok[b] with failing[B] = 0 behind them -- the exclusive sum of these B + 1
// entries gives every failing trial its place in the compacted batch and, in entry B, their number.
template <int DC>
__global__ void __launch_bounds__(256) k_choi_is_cptp(const double* __restrict__ choi, int B, double atol, int32_t* __restrict__ ok,
                                                      int32_t* __restrict__ failing) {
  using W = StatesChoi<DC>;
  constexpr int d = W::d, D = W::D, LD = W::LD;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int t = threadIdx.x, slot = t / W::TT, u = t % W::TT;
  const int b = blockIdx.x * W::TPB + slot;
  const bool live = b < B;
  cd* A = reinterpret_cast<cd*>(smem) + (size_t)slot * (D * LD + 1);
  int* bad = reinterpret_cast<int*>(A + D * LD);  // any thread of the trial sets it; read after the last barrier
  // (a slot past the batch reads trial B - 1 and writes nothing: its threads still reach every barrier)
  const cd* src = reinterpret_cast<const cd*>(choi) + (size_t)(live ? b : B - 1) * D * D;
  if (u == 0) *bad = 0;
  __syncthreads();
  bool mine = false;
  // the Hermitian part, shifted by atol, into the image; the finite check on the raw entries
  for (int e = u; e < D * D; e += W::TT) {
    const int i = e / D, j = e % D;
    const cd a = src[e], c = src[j * D + i];
    if (!(fabs(a.re) <= 1.79769313486231570e308 && fabs(a.im) <= 1.79769313486231570e308)) mine = true;
    cd hpart{0.5 * (a.re + c.re), 0.5 * (a.im - c.im)};
    if (i == j) hpart.re += atol;
    A[i * LD + j] = hpart;
  }
  // trace preservation on the raw entries: thread u < d^2 owns R[i][j]
  if (u < d * d) {
    const int i = u / d, j = u % d;
    double sr = 0.0, si = 0.0;
    for (int k = 0; k < d; ++k) {
      const cd a = src[(i * d + k) * D + j * d + k];
      sr += a.re;
      si += a.im;
    }
    const double one = i == j ? 1.0 : 0.0;
    if (!(hypot(sr - one, si) <= atol + 1e-5 * one)) mine = true;
  }
  __syncthreads();
  // L D L^H, right-looking: step k reads column k (final since step k - 1) and updates the lower triangle behind it
  for (int k = 0; k < D; ++k) {
    const double piv = A[k * LD + k].re;
    const bool pos = piv > 0.0;  // (a NaN is not)
    if (!pos) mine = true;
    const double inv = pos ? 1.0 / piv : 0.0;
    for (int e = u; e < D * D; e += W::TT) {
      const int i = e / D, j = e % D;
      if (j > k && i >= j) {
        const cd x = A[i * LD + k], y = A[j * LD + k];
        cd v = A[i * LD + j];
        v.re -= (x.re * y.re + x.im * y.im) * inv;
        v.im -= (x.im * y.re - x.re * y.im) * inv;
        A[i * LD + j] = v;
      }
    }
    __syncthreads();
  }
  if (mine) *bad = 1;
  __syncthreads();
  if (live && u == 0) {
    ok[b] = *bad ? 0 : 1;
    if (failing) failing[b] = *bad ? 1 : 0;
  }
  if (failing && blockIdx.x == 0 && t == 0) failing[B] = 0;
}

// The failing trials' matrices, in batch order, into `packed` (pos: the exclusive sum of `failing`)
template <int DC>
__global__ void __launch_bounds__(256) k_choi_gather(const double* __restrict__ choi, int B, const int32_t* __restrict__ ok,
                                                     const int32_t* __restrict__ pos, double* __restrict__ packed) {
  constexpr int ne2 = 2 * StatesChoi<DC>::D * StatesChoi<DC>::D;  // doubles per matrix
  const int b = blockIdx.x;
  if (b >= B || ok[b]) return;
  const double2* src = reinterpret_cast<const double2*>(choi + (size_t)b * ne2);
  double2* dst = reinterpret_cast<double2*>(packed + (size_t)pos[b] * ne2);
  for (int e = threadIdx.x; e < ne2 / 2; e += 256) dst[e] = src[e];
}

// ... and the projected matrices back to their trials.  projected[b] = 1 - ok[b] and iters[b] (0 for a passing trial) are
// written for every trial; both may be null.
template <int DC>
__global__ void __launch_bounds__(256) k_choi_scatter(const double* __restrict__ packed, const int32_t* __restrict__ packed_iters,
                                                      int B, const int32_t* __restrict__ ok, const int32_t* __restrict__ pos,
                                                      double* __restrict__ choi, int32_t* __restrict__ projected,
                                                      int32_t* __restrict__ iters) {
  constexpr int ne2 = 2 * StatesChoi<DC>::D * StatesChoi<DC>::D;
  const int b = blockIdx.x;
  if (b >= B) return;
  const bool failed = !ok[b];
  if (threadIdx.x == 0) {
    if (projected) projected[b] = failed;
    if (iters) iters[b] = failed ? packed_iters[pos[b]] : 0;
  }
  if (!failed) return;
  const double2* src = reinterpret_cast<const double2*>(packed + (size_t)pos[b] * ne2);
  double2* dst = reinterpret_cast<double2*>(choi + (size_t)b * ne2);
  for (int e = threadIdx.x; e < ne2 / 2; e += 256) dst[e] = src[e];
}

}  // namespace qt
