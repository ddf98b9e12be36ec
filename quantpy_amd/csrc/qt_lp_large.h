// qt_lp_large.h -- qt_lp.h's batch of dense linear programs for 65 ... 255 variables (qt_lp_ineq_large_batch):
//
//     for r < R, o < O:  minimise C[o] . x  subject to  A x <= b[r],  x in R^N free   (N <= 255, any M >= N)
//
// The programs are the process polytope of PolytopeProcessInterval at n = 2 (reference interval.py:338-418; A is
// 576 x 240 with 'sic' inputs and 'proj-set') and the state polytope at n = 4 (1296 x 255).  The iteration and the
// per-workgroup driver are qt_lp.h's lp_phase and lp_run, the same text for both kernels; this file holds the primitives
// they run on here and the struct (LpLarge) that hands them over.  What the primitives do differently:
//
//   * The normal matrix (n x n, n <= 256 with the phase-1 column) does not fit LDS.  It lives in this workgroup's slice
//     of a global workspace (512 KB: it stays in L2 / Infinity Cache), row stride kLgLD.
//   * H = A^T diag(w) A is formed in two passes over A, each through LDS row blocks of kLgRB rows: a pass keeps five of
//     the ten 64 x 64 blocks of the lower triangle in registers (4 x 4 per thread and block).  The phase-1 column (-1 in
//     every row) is written into the LDS block, so the bordered matrix needs no pass of its own.
//   * Cholesky is blocked (right-looking, kLgNB = 32 columns): the diagonal block is factored in LDS, every thread then
//     solves one row of the panel in its own LDS row, and the trailing matrix is updated in 4 x 4 register tiles from the panel
//     in LDS -- 8 panels instead of 255 rank-1 updates over global memory.
//   * A safeguard: a pivot of the factorisation that is not above kLgPivot of its diagonal entry of H is replaced by
//     that entry (the row then hardly moves in the solve).  Without it the iteration breaks down on most of the polytope
//     programs of this size (a non-positive pivot a few iterations before the end, with the gap already at
//     1e-10 ... 5e-8).  A factorisation without such a pivot is computed as before, so a program that never breaks down
//     is not touched; a replaced pivot perturbs the Newton direction, not the residuals, which are recomputed from A
//     every iteration.  tests/lp_model.py is the NumPy model in which this was compared with HiGHS -- and in which a
//     fixed shift H + 1e-12 diag(H) on every factorisation stalled a program that needs no safeguard at all.
//   * The triangular solves are blocked the same way: one wavefront solves a 32 x 32 diagonal block from LDS with
//     shuffles, all threads then update the rest of the vector from global memory (3 barriers per block).
//   * A y is one wavefront per row (coalesced, butterfly sum) into a seventh M-vector; A^T v is one thread per column.
//
// Every loop has a bound; every branch that contains a barrier depends only on values that are uniform over the
// workgroup; the rank test of A^T A runs once per workgroup.
#pragma once

#include "qt_lp.h"

namespace qt {

constexpr int kLgMaxN = 255;      // variables; phase 1 adds t
constexpr int kLgLD = 256;        // row stride of the normal matrix in global memory
constexpr int kLgRB = 16;         // rows of A per LDS block while forming H
constexpr int kLgNB = 32;         // Cholesky panel width
constexpr int kLgDS = kLgNB + 1;  // LDS row stride of a panel / diagonal block
constexpr double kLgPivot = 1e-11;  // a pivot not above this fraction of its diagonal entry is replaced
constexpr size_t kLgHDoubles = (size_t)kLgLD * kLgLD;

struct LgShared {
  // the row block of A (kLgRB x kLgLD) while forming H; the Cholesky panel (<= 224 rows, stride kLgDS) otherwise
  double buf[(kLgLD - kLgNB) * kLgDS];
  double D[kLgNB * kLgDS];
  double y[kLgLD], dy[kLgLD], rd[kLgLD], u[kLgLD], c[kLgLD], diag[kLgLD];
  double red[4 * 4];
};

// out[i] = a_i . y over the first N columns: one wavefront per row, four rows in flight.  No barrier inside.
__device__ inline void lg_matvec(const double* __restrict__ A, int M, int N, const double* y, double* out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int i0 = w; i0 < M; i0 += 16) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < N; j += 64) {
      const double yj = y[j];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + 4 * q;
        if (i < M) acc[q] = fma(A[(size_t)i * N + j], yj, acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      for (int off = 32; off > 0; off >>= 1) acc[q] += __shfl_xor(acc[q], off, 64);
    if (lane == 0)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + 4 * q < M) out[i0 + 4 * q] = acc[q];
  }
}

// sh.u[j] = sum_i A[i][j] v[i] (j < N) and, in phase 1, sh.u[N] = sum_i v[i] (phase 2 never reads it); v is global,
// written by other threads before the call.  One thread per column; the sum of v is a workgroup reduction.
__device__ inline void lg_colsum(LgShared& sh, const double* __restrict__ A, int M, int N, const double* v, bool p1) {
  __syncthreads();
  const int t = threadIdx.x;
  if (t < N) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int i = 0;
    for (; i + 3 < M; i += 4) {
      a0 = fma(A[(size_t)i * N + t], v[i], a0);
      a1 = fma(A[(size_t)(i + 1) * N + t], v[i + 1], a1);
      a2 = fma(A[(size_t)(i + 2) * N + t], v[i + 2], a2);
      a3 = fma(A[(size_t)(i + 3) * N + t], v[i + 3], a3);
    }
    for (; i < M; ++i) a0 = fma(A[(size_t)i * N + t], v[i], a0);
    sh.u[t] = (a0 + a1) + (a2 + a3);
  }
  if (p1) {  // uniform
    double tot[1] = {0.0};
    for (int i = t; i < M; i += kLpNT) tot[0] += v[i];
    lp_reduce<1, false>(tot, sh.red);
    if (t == 0) sh.u[N] = tot[0];
  }
  __syncthreads();
}

// acc += p q^T (4 x 4) / its write-out to block (bi, bj) of H; the block is skipped when it lies beyond column n
#define QT_LG_FMA(acc, p, q, bi)                                          \
  if (64 * (bi) < n) {                                                    \
    _Pragma("unroll") for (int a = 0; a < 4; ++a)                         \
      _Pragma("unroll") for (int b = 0; b < 4; ++b) acc[a][b] = fma(p[a], q[b], acc[a][b]); \
  }
#define QT_LG_OUT(acc, bi, bj)                                            \
  _Pragma("unroll") for (int a = 0; a < 4; ++a)                           \
    _Pragma("unroll") for (int b = 0; b < 4; ++b) {                       \
      const int i = 64 * (bi) + 4 * tj + a, j = 64 * (bj) + 4 * tk + b;   \
      if (i < n && j < n) H[(size_t)i * kLgLD + j] = acc[a][b];           \
    }

// One pass of H = A^T diag(w) A over the n = N + p1 columns (column N is -1 in every row), over LDS row blocks of A.
// A pass keeps five 64 x 64 blocks (bi, bj) of the lower triangle in registers, 4 x 4 per thread and block:
// pass 0 (0,0) (1,0) (1,1) (2,0) (2,1), pass 1 (2,2) (3,0) (3,1) (3,2) (3,3).
template <int PASS>
__device__ inline void lg_normal_pass(LgShared& sh, const double* __restrict__ A, int M, int N, int n, bool p1,
                                      const double* w, double* __restrict__ H) {
  const int t = threadIdx.x, tj = t >> 4, tk = t & 15;
  double* wblk = sh.D;  // kLgRB weights; sh.D is free while H is formed
  double acc0[4][4] = {}, acc1[4][4] = {}, acc2[4][4] = {}, acc3[4][4] = {}, acc4[4][4] = {};
  for (int r0 = 0; r0 < M; r0 += kLgRB) {
    __syncthreads();
    for (int e = t; e < kLgRB * kLgLD; e += kLpNT) {
      const int r = e / kLgLD, j = e % kLgLD, i = r0 + r;
      double a = 0.0;
      if (i < M) a = (j < N) ? A[(size_t)i * N + j] : ((p1 && j == N) ? -1.0 : 0.0);
      sh.buf[e] = a;
    }
    if (t < kLgRB) wblk[t] = (r0 + t < M) ? w[r0 + t] : 0.0;
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < kLgRB; ++r) {
      const double* row = sh.buf + r * kLgLD;
      const double dr = wblk[r];
      double p0[4], p1v[4], p2[4], p3[4], q0[4], q1[4], q2[4], q3[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        p0[a] = dr * row[4 * tj + a];
        p1v[a] = dr * row[64 + 4 * tj + a];
        p2[a] = dr * row[128 + 4 * tj + a];
        p3[a] = dr * row[192 + 4 * tj + a];
        q0[a] = row[4 * tk + a];
        q1[a] = row[64 + 4 * tk + a];
        q2[a] = row[128 + 4 * tk + a];
        q3[a] = row[192 + 4 * tk + a];
      }
      if constexpr (PASS == 0) {
        QT_LG_FMA(acc0, p0, q0, 0)
        QT_LG_FMA(acc1, p1v, q0, 1)
        QT_LG_FMA(acc2, p1v, q1, 1)
        QT_LG_FMA(acc3, p2, q0, 2)
        QT_LG_FMA(acc4, p2, q1, 2)
      } else {
        QT_LG_FMA(acc0, p2, q2, 2)
        QT_LG_FMA(acc1, p3, q0, 3)
        QT_LG_FMA(acc2, p3, q1, 3)
        QT_LG_FMA(acc3, p3, q2, 3)
        QT_LG_FMA(acc4, p3, q3, 3)
      }
    }
  }
  if constexpr (PASS == 0) {
    QT_LG_OUT(acc0, 0, 0)
    QT_LG_OUT(acc1, 1, 0)
    QT_LG_OUT(acc2, 1, 1)
    QT_LG_OUT(acc3, 2, 0)
    QT_LG_OUT(acc4, 2, 1)
  } else {
    QT_LG_OUT(acc0, 2, 2)
    QT_LG_OUT(acc1, 3, 0)
    QT_LG_OUT(acc2, 3, 1)
    QT_LG_OUT(acc3, 3, 2)
    QT_LG_OUT(acc4, 3, 3)
  }
}
#undef QT_LG_FMA
#undef QT_LG_OUT

__device__ __noinline__ void lg_normal(LgShared& sh, const double* __restrict__ A, int M, int N, bool p1, const double* w,
                                 double* __restrict__ H) {
  const int n = N + (p1 ? 1 : 0);
  lg_normal_pass<0>(sh, A, M, N, n, p1, w, H);
  if (n > 128) lg_normal_pass<1>(sh, A, M, N, n, p1, w, H);
  __syncthreads();
}

// sh.D <- the lower triangle of the diagonal block at k0 (nb x nb), padded with the identity to kLgNB x kLgNB
__device__ inline void lg_load_diag(LgShared& sh, const double* H, int k0, int nb) {
  for (int e = threadIdx.x; e < kLgNB * kLgNB; e += kLpNT) {
    const int i = e / kLgNB, j = e % kLgNB;
    sh.D[i * kLgDS + j] = (i < nb && j <= i) ? H[(size_t)(k0 + i) * kLgLD + k0 + j] : (i == j ? 1.0 : 0.0);
  }
}

// In-place blocked Cholesky of the lower triangle of H (n x n, global).  A pivot that is not above rel * (its diagonal
// entry before the factorisation) is replaced by that entry (replace) or is a breakdown; so is one that is not
// finite, or a diagonal entry that is not positive.  A breakdown returns false (the same answer in every thread).
__device__ inline bool lg_cholesky(LgShared& sh, double* H, int n, double rel, bool replace) {
  const int t = threadIdx.x, tj = t >> 4, tk = t & 15;
  __syncthreads();
  if (t < n) sh.diag[t] = H[(size_t)t * kLgLD + t];
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += kLgNB) {
    const int nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    lg_load_diag(sh, H, k0, nb);
    __syncthreads();
    for (int k = 0; k < nb; ++k) {
      double p = sh.D[k * kLgDS + k];
      const double d = sh.diag[k0 + k];
      if (!isfinite(p) || !isfinite(d) || !(d > 0.0)) return false;
      if (!(p > rel * d)) {
        if (!replace) return false;
        p = d;
      }
      const double l = sqrt(p);
      __syncthreads();  // every thread has read the pivot
      if (t < nb - k) sh.D[(k + t) * kLgDS + k] = (t == 0) ? l : sh.D[(k + t) * kLgDS + k] / l;
      __syncthreads();
      for (int e = t; e < kLgNB * kLgNB; e += kLpNT) {
        const int i = e / kLgNB, j = e % kLgNB;
        if (j > k && j <= i && i < nb)
          sh.D[i * kLgDS + j] = fma(-sh.D[i * kLgDS + k], sh.D[j * kLgDS + k], sh.D[i * kLgDS + j]);
      }
      __syncthreads();
    }
    for (int e = t; e < kLgNB * kLgNB; e += kLpNT) {
      const int i = e / kLgNB, j = e % kLgNB;
      if (i < nb && j <= i) H[(size_t)(k0 + i) * kLgLD + k0 + j] = sh.D[i * kLgDS + j];
    }
    const int m = n - k0 - nb;  // rows below the panel (<= 224)
    if (m > 0) {
      // panel: row i of L21 = H21 L11^-T, one row per thread, kept in the thread's own row of sh.buf
      if (t < m) {
        double* hrow = H + (size_t)(k0 + nb + t) * kLgLD + k0;
        double* r = sh.buf + t * kLgDS;
        for (int k = 0; k < kLgNB; ++k) r[k] = (k < nb) ? hrow[k] : 0.0;
#pragma unroll 1
        for (int k = 0; k < nb; ++k) {
          const double* dk = sh.D + k * kLgDS;
          double a = r[k];
          for (int j = 0; j < k; ++j) a = fma(-r[j], dk[j], a);
          a /= dk[k];
          r[k] = a;
          hrow[k] = a;
        }
      }
      __syncthreads();
      // trailing matrix: H22 -= L21 L21^T, lower triangle, 64 x 64 blocks in 4 x 4 register tiles
      double* H22 = H + (size_t)(k0 + nb) * kLgLD + (k0 + nb);
      for (int bi = 0; 64 * bi < m; ++bi)
        for (int bj = 0; bj <= bi; ++bj) {
          const int ri = 64 * bi + 4 * tj, rj = 64 * bj + 4 * tk;
          double acc[4][4] = {};
#pragma unroll 4
          for (int k = 0; k < kLgNB; ++k) {
            double p[4], q[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) p[a] = (ri + a < m) ? sh.buf[(ri + a) * kLgDS + k] : 0.0;
#pragma unroll
            for (int b = 0; b < 4; ++b) q[b] = (rj + b < m) ? sh.buf[(rj + b) * kLgDS + k] : 0.0;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b) acc[a][b] = fma(p[a], q[b], acc[a][b]);
          }
#pragma unroll
          for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
              if (ri + a < m && rj + b <= ri + a) H22[(size_t)(ri + a) * kLgLD + rj + b] -= acc[a][b];
        }
      __syncthreads();
    }
  }
  __syncthreads();  // the last diagonal block is in H, sh.D is free
  return true;
}

// v <- (L L^T)^{-1} v for the factor in H; v is in LDS, written before the caller's last barrier
__device__ __noinline__ void lg_solve(LgShared& sh, const double* H, int n, double* v) {
  const int t = threadIdx.x, lane = t & 63;
  const int nblk = (n + kLgNB - 1) / kLgNB;
  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = kb * kLgNB, nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    lg_load_diag(sh, H, k0, nb);
    __syncthreads();
    if (t < 64) {
      double val = (lane < nb) ? v[k0 + lane] : 0.0;
#pragma unroll
      for (int k = 0; k < kLgNB; ++k) {
        const double vk = __shfl(val, k, 64) / sh.D[k * kLgDS + k];
        if (lane == k)
          val = vk;
        else if (lane > k && lane < kLgNB)
          val = fma(-sh.D[lane * kLgDS + k], vk, val);
      }
      if (lane < nb) v[k0 + lane] = val;
    }
    __syncthreads();
    const int i = k0 + nb + t;
    if (i < n) {
      const double* hrow = H + (size_t)i * kLgLD + k0;
      double acc = v[i];
      for (int k = 0; k < nb; ++k) acc = fma(-hrow[k], v[k0 + k], acc);
      v[i] = acc;
    }
    __syncthreads();
  }
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int k0 = kb * kLgNB, nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    lg_load_diag(sh, H, k0, nb);
    __syncthreads();
    if (t < 64) {
      double val = (lane < nb) ? v[k0 + lane] : 0.0;
#pragma unroll
      for (int k = kLgNB - 1; k >= 0; --k) {
        const double vk = __shfl(val, k, 64) / sh.D[k * kLgDS + k];
        if (lane == k)
          val = vk;
        else if (lane < k)
          val = fma(-sh.D[k * kLgDS + lane], vk, val);
      }
      if (lane < nb) v[k0 + lane] = val;
    }
    __syncthreads();
    if (t < k0) {
      double acc = v[t];
      for (int k = 0; k < nb; ++k) acc = fma(-H[(size_t)(k0 + k) * kLgLD + t], v[k0 + k], acc);
      v[t] = acc;
    }
    __syncthreads();
  }
}

// k_lp_ineq_large's primitives for lp_phase / lp_run (see LpSmall): the normal matrix at the head of the workgroup's
// workspace, A v through a seventh M-vector behind the six of the iteration.
struct LpLarge {
  using Shared = LgShared;
  static constexpr int kCols = kLgLD;
  const double* __restrict__ A;
  int M, N;
  double *H, *vec, *ax;

  __host__ __device__ static size_t ws_doubles(int M) { return kLgHDoubles + (size_t)7 * M; }
  __device__ LpLarge(const double* A, int M, int N, double* ws)
      : A(A), M(M), N(N), H(ws), vec(ws + kLgHDoubles), ax(vec + (size_t)6 * M) {}
  __device__ __forceinline__ void matvec(const double* v) const {
    lg_matvec(A, M, N, v, ax);
    __syncthreads();
  }
  // phase 2 starts from the ax that phase 1's last matvec(sh.y) left here
  __device__ __forceinline__ double av(int i, const double*) const { return ax[i]; }
  __device__ __forceinline__ void colsum(LgShared& sh, const double* v, bool p1) const { lg_colsum(sh, A, M, N, v, p1); }
  __device__ __forceinline__ void normal(LgShared& sh, const double* w, bool p1) const {
    lg_normal(sh, A, M, N, p1, w, H);  // its first barrier orders the writes of w
  }
  __device__ __forceinline__ bool factor(LgShared& sh, const double* w, bool p1) const {
    normal(sh, w, p1);
    return lg_cholesky(sh, H, N + (p1 ? 1 : 0), kLgPivot, true);
  }
  __device__ __forceinline__ bool full_rank(LgShared& sh, const double* w) const {
    normal(sh, w, false);
    return lg_cholesky(sh, H, N, 1e-12, false);
  }
  __device__ __forceinline__ void solve(LgShared& sh, int n, double* v) const { lg_solve(sh, H, n, v); }
  __device__ __forceinline__ double h_at(const LgShared&, int i, int j) const { return H[(size_t)i * kLgLD + j]; }
};

#ifndef QT_LP_PRIMITIVES_ONLY  // qt_lp_pieces.hip takes the primitives without the kernel (one definition per library)
// grid: persistent workgroups over the R * O programs; ws: gridDim.x * LpLarge::ws_doubles(M) doubles
__global__ void __launch_bounds__(kLpNT) k_lp_ineq_large(const double* __restrict__ A, int M, int N,
                                                         const double* __restrict__ C, int O,
                                                         const double* __restrict__ bb, int R, double* __restrict__ obj,
                                                         double* __restrict__ xout, int32_t* __restrict__ status,
                                                         int32_t* __restrict__ iters, double* __restrict__ ws) {
  __shared__ LgShared sh;
  lp_run(sh, LpLarge(A, M, N, ws + blockIdx.x * LpLarge::ws_doubles(M)), C, O, bb, R, obj, xout, status, iters);
}
#endif

}  // namespace qt
