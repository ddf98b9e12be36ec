// qt_lp_xl.h -- qt_lp.h's batch of dense linear programs for up to 1023 variables (qt_lp_ineq_xl_batch):
//
//     for r < R, o < O:  minimise C[o] . x  subject to  A x <= b[r],  x in R^N free   (N <= 1023, any M >= N)
//
// The programs are the state polytope of PolytopeStateInterval at n = 5 (reference interval.py:268-335; A is
// 7776 x 1023 with 'proj-set').  The iteration and the per-workgroup driver are qt_lp.h's lp_phase and lp_run, the same
// text for three kernels; this file holds the primitives they run on here and the struct (LpXl) that hands them over.
// They follow qt_lp_large.h's, with these differences:
//
//   * The normal matrix (n x n, n <= 1024 with the phase-1 column) is 8 MB, in this workgroup's slice of the global
//     workspace, row stride kXlLD.  The six n-vectors of the iteration are 48 KB of LDS and are walked in strides of
//     the workgroup (QT_LP_COLS).
//   * H = A^T diag(w) A is where the time goes (4.1 G multiply-adds at 7776 x 1024).  xl_syrk forms the lower triangle
//     in 128 x 128 blocks on the FP64 matrix cores: a wavefront keeps a 64 x 64 quarter as sixteen 16 x 16
//     accumulators of v_mfma_f64_16x16x4_f64, the operands come from LDS row blocks of kXlRB rows of A (the 128
//     columns of the block's rows, weighted, beside the 128 of its columns), and the next row block is loaded into
//     registers while the products of this one run.  The 36 blocks of the triangle read 8 x 1024 columns of A in all:
//     eight passes.  The phase-1 column (-1 in every row) is written into the LDS block.
//   * Cholesky is blocked as in qt_lp_large.h (kLgNB = 32 columns, the same diagonal-block code and safeguard
//     kLgPivot); a thread solves its panel rows (every 256th) in its own LDS row, and the trailing update
//     H22 -= L21 L21^T is the same xl_syrk, the panel read from H with k running fastest.
//   * The triangular solves are qt_lp_large.h's with the vector updates strided; A^T v is one wavefront per fourth row
//     and sixteen columns per lane, summed over the four wavefronts in LDS; A y is lg_matvec itself.
//
// Every loop has a bound; every branch that contains a barrier depends only on values that are uniform over the
// workgroup; workgroups do not talk to each other; the rank test of A^T A runs once per workgroup.
#pragma once

#include "qt_lp_large.h"

namespace qt {

constexpr int kXlMaxN = 1023;      // variables; phase 1 adds t
constexpr int kXlLD = 1024;        // row stride of the normal matrix in global memory
constexpr int kXlRB = 16;          // rows of A per LDS block while forming H
constexpr int kXlSB = 128;         // xl_syrk's block of H: 2 x 2 wavefronts of 64 x 64
constexpr int kXlBS = 2 * kXlSB + 16;  // LDS row stride of a row block: rows k, k + 1 of an operand fall in different halves of the banks
constexpr size_t kXlHDoubles = (size_t)kXlLD * kXlLD;

typedef double xl_v4f64 __attribute__((ext_vector_type(4)));

struct XlShared {
  // the row block of xl_syrk (kXlRB x kXlBS); the panel rows of a sweep (kLpNT rows, stride kLgDS); xl_colsum's partial sums
  double buf[kLpNT * kLgDS];
  double D[kLgNB * kLgDS];
  double y[kXlLD], dy[kXlLD], rd[kXlLD], u[kXlLD], c[kXlLD], diag[kXlLD];
  double red[4 * 4];
};
static_assert(kXlRB * kXlBS <= kLpNT * kLgDS && 4 * kXlLD <= kLpNT * kLgDS, "XlShared::buf holds a row block and the column partials");

// sh.u[j] = sum_i A[i][j] v[i] (j < N) and, in phase 1, sh.u[N] = sum_i v[i]; v is global, written by other threads
// before the call.  Wavefront g takes rows g, g + 4, ...; a lane the columns lane + 64 c.
__device__ inline void xl_colsum(XlShared& sh, const double* __restrict__ A, int M, int N, const double* v, bool p1) {
  __syncthreads();
  const int t = threadIdx.x, lane = t & 63, g = t >> 6;
  double acc[kXlLD / 64] = {};
#pragma unroll 2
  for (int i = g; i < M; i += 4) {
    const double vi = v[i];
    const double* __restrict__ row = A + (size_t)i * N;
#pragma unroll
    for (int c = 0; c < kXlLD / 64; ++c) {
      const int j = lane + 64 * c;
      if (64 * c < N) {  // uniform; a lane past column N rereads column 0 and drops it: no branch per lane
        const double a = row[j < N ? j : 0];
        acc[c] = fma(j < N ? a : 0.0, vi, acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kXlLD / 64; ++c) sh.buf[g * kXlLD + lane + 64 * c] = acc[c];
  __syncthreads();
  for (int j = t; j < N; j += kLpNT)
    sh.u[j] = (sh.buf[j] + sh.buf[kXlLD + j]) + (sh.buf[2 * kXlLD + j] + sh.buf[3 * kXlLD + j]);
  if (p1) {  // uniform
    double tot[1] = {0.0};
    for (int i = t; i < M; i += kLpNT) tot[0] += v[i];
    lp_reduce<1, false>(tot, sh.red);
    if (t == 0) sh.u[N] = tot[0];
  }
  __syncthreads();
}

// The lower triangle of G[i][j] = sum_{k < K} w[k] S(k, i) S(k, j), i, j < m, into H (row stride kXlLD): H = G, or
// H -= G (UPDATE).  load(k, col) is S for k < K, col < m; w may be null (all one).  KFAST says which index of S runs
// fastest in memory, so that neighbouring threads load neighbouring addresses.  Blocks of kXlSB x kXlSB, each summed over
// LDS row blocks of kXlRB values of k: columns 0 ... 127 of a row block are w S at the block's rows i, 128 ... 255 are S
// at its columns j.  Wavefront (wi, wj) owns the 64 x 64 quarter, as 4 x 4 accumulators of the 16 x 16 x 4 product
// (operand lane l: row / column l & 15, k = l >> 4; result register r: row (l >> 4) + 4 r, column l & 15).
// Known waste, left for a measurement of where an iteration's 187 ms go (profiles/lp_xl_timing.txt): a diagonal block
// stages its 128 columns twice and its wavefront (0, 1) idles (8 of the 36 blocks at n = 1024), and a block that
// reaches past column m (the last one, or a trailing update with few rows) multiplies its zero tiles like the others.
template <bool UPDATE, bool KFAST, class Load>
__device__ __forceinline__ void xl_syrk(XlShared& sh, int m, int K, Load load, const double* w, double* __restrict__ H) {
  const int t = threadIdx.x, lane = t & 63, wi = t >> 7, wj = (t >> 6) & 1;
  constexpr int kPer = kXlRB * 2 * kXlSB / kLpNT;  // values of a row block per thread
  for (int bi = 0; kXlSB * bi < m; ++bi)
    for (int bj = 0; bj <= bi; ++bj) {
      xl_v4f64 acc[4][4];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = xl_v4f64{0.0, 0.0, 0.0, 0.0};
      double pre[kPer];
      auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
          const int e = t + kLpNT * q;
          const int r = KFAST ? e % kXlRB : e / (2 * kXlSB), c = KFAST ? e / kXlRB : e % (2 * kXlSB);
          const int k = k0 + r, col = (c < kXlSB) ? kXlSB * bi + c : kXlSB * bj + (c - kXlSB);
          // no branch around the loads: outside the range S(0, 0) is read and dropped (K, m >= 1)
          const bool in = k < K && col < m;
          const int kc = in ? k : 0;
          double v = load(kc, in ? col : 0);
          if (w) {  // uniform
            const double wk = w[kc];
            v *= (c < kXlSB) ? wk : 1.0;
          }
          pre[q] = in ? v : 0.0;
        }
      };
      fetch(0);
      const bool mine = !(bi == bj && wi < wj);  // the quarter above the diagonal is never written
      for (int k0 = 0; k0 < K; k0 += kXlRB) {
        __syncthreads();  // the last row block has been read
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
          const int e = t + kLpNT * q;
          const int r = KFAST ? e % kXlRB : e / (2 * kXlSB), c = KFAST ? e / kXlRB : e % (2 * kXlSB);
          sh.buf[r * kXlBS + c] = pre[q];
        }
        __syncthreads();
        if (k0 + kXlRB < K) fetch(k0 + kXlRB);  // uniform; in flight during the products
        if (mine) {  // uniform over the wavefront, no barrier inside
#pragma unroll
          for (int kk = 0; kk < kXlRB; kk += 4) {
            const double* row = sh.buf + (kk + (lane >> 4)) * kXlBS + (lane & 15);
            double p[4], q[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) p[a] = row[64 * wi + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) q[b] = row[kXlSB + 64 * wj + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(p[a], q[b], acc[a][b], 0, 0, 0);
          }
        }
      }
      if (mine) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = kXlSB * bi + 64 * wi + 16 * a + (lane >> 4) + 4 * r, j = kXlSB * bj + 64 * wj + 16 * b + (lane & 15);
              if (i < m && j <= i) {
                double* h = H + (size_t)i * kXlLD + j;
                *h = UPDATE ? *h - acc[a][b][r] : acc[a][b][r];
              }
            }
      }
    }
}

// H = A^T diag(w) A over the n = N + p1 columns (column N is -1 in every row)
__device__ __forceinline__ void xl_normal(XlShared& sh, const double* __restrict__ A, int M, int N, bool p1, const double* w,
                                       double* __restrict__ H) {
  xl_syrk<false, false>(sh, N + (p1 ? 1 : 0), M, [=](int k, int col) { return col < N ? A[(size_t)k * N + col] : -1.0; }, w, H);
  __syncthreads();
}

// sh.D <- the lower triangle of the diagonal block at k0 (nb x nb), padded with the identity to kLgNB x kLgNB
__device__ inline void xl_load_diag(XlShared& sh, const double* H, int k0, int nb) {
  for (int e = threadIdx.x; e < kLgNB * kLgNB; e += kLpNT) {
    const int i = e / kLgNB, j = e % kLgNB;
    sh.D[i * kLgDS + j] = (i < nb && j <= i) ? H[(size_t)(k0 + i) * kXlLD + k0 + j] : (i == j ? 1.0 : 0.0);
  }
}

// lg_cholesky for n <= 1024: in-place blocked Cholesky of the lower triangle of H (n x n, global), the same pivot
// rules.  A breakdown returns false (the same answer in every thread).
__device__ __forceinline__ bool xl_cholesky(XlShared& sh, double* H, int n, double rel, bool replace) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int j = t; j < n; j += kLpNT) sh.diag[j] = H[(size_t)j * kXlLD + j];
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += kLgNB) {
    const int nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    xl_load_diag(sh, H, k0, nb);
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
      if (i < nb && j <= i) H[(size_t)(k0 + i) * kXlLD + k0 + j] = sh.D[i * kLgDS + j];
    }
    const int m = n - k0 - nb;  // rows below the panel; nb = kLgNB when there are any
    if (m > 0) {
      // panel: row i of L21 = H21 L11^-T, in the thread's own row of sh.buf.  A thread reads 32 doubles of its own row
      // of H, 8 KB from its neighbour's (as in xl_solve's forward sweep): not coalesced, and not measured on its own
      for (int i = t; i < m; i += kLpNT) {
        double* hrow = H + (size_t)(k0 + nb + i) * kXlLD + k0;
        double* r = sh.buf + t * kLgDS;
        for (int k = 0; k < kLgNB; ++k) r[k] = hrow[k];
#pragma unroll 1
        for (int k = 0; k < kLgNB; ++k) {
          const double* dk = sh.D + k * kLgDS;
          double a = r[k];
          for (int j = 0; j < k; ++j) a = fma(-r[j], dk[j], a);
          a /= dk[k];
          r[k] = a;
          hrow[k] = a;
        }
      }
      __syncthreads();  // the panel is in H; sh.buf and sh.D are free
      // trailing matrix: H22 -= L21 L21^T, lower triangle
      const double* L21 = H + (size_t)(k0 + nb) * kXlLD + k0;
      xl_syrk<true, true>(sh, m, kLgNB, [=](int k, int col) { return L21[(size_t)col * kXlLD + k]; }, nullptr,
                          H + (size_t)(k0 + nb) * kXlLD + (k0 + nb));
      __syncthreads();
    }
  }
  __syncthreads();  // the last diagonal block is in H, sh.D is free
  return true;
}

// lg_solve for n <= 1024: v <- (L L^T)^{-1} v for the factor in H; v is in LDS, written before the caller's last barrier
__device__ __forceinline__ void xl_solve(XlShared& sh, const double* H, int n, double* v) {
  const int t = threadIdx.x, lane = t & 63;
  const int nblk = (n + kLgNB - 1) / kLgNB;
  for (int kb = 0; kb < nblk; ++kb) {
    const int k0 = kb * kLgNB, nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    xl_load_diag(sh, H, k0, nb);
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
    for (int i = k0 + nb + t; i < n; i += kLpNT) {
      const double* hrow = H + (size_t)i * kXlLD + k0;
      double acc = v[i];
      for (int k = 0; k < nb; ++k) acc = fma(-hrow[k], v[k0 + k], acc);
      v[i] = acc;
    }
    __syncthreads();
  }
  for (int kb = nblk - 1; kb >= 0; --kb) {
    const int k0 = kb * kLgNB, nb = (n - k0 < kLgNB) ? n - k0 : kLgNB;
    xl_load_diag(sh, H, k0, nb);
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
    for (int i = t; i < k0; i += kLpNT) {
      double acc = v[i];
      for (int k = 0; k < nb; ++k) acc = fma(-H[(size_t)(k0 + k) * kXlLD + i], v[k0 + k], acc);
      v[i] = acc;
    }
    __syncthreads();
  }
}

// k_lp_ineq_xl's primitives for lp_phase / lp_run (see LpSmall): LpLarge's layout with an 8 MB normal matrix.
struct LpXl {
  using Shared = XlShared;
  static constexpr int kCols = kXlLD;
  const double* __restrict__ A;
  int M, N;
  double *H, *vec, *ax;

  __host__ __device__ static size_t ws_doubles(int M) { return kXlHDoubles + (size_t)7 * M; }
  __device__ LpXl(const double* A, int M, int N, double* ws)
      : A(A), M(M), N(N), H(ws), vec(ws + kXlHDoubles), ax(vec + (size_t)6 * M) {}
  __device__ __forceinline__ void matvec(const double* v) const {
    lg_matvec(A, M, N, v, ax);
    __syncthreads();
  }
  // phase 2 starts from the ax that phase 1's last matvec(sh.y) left here
  __device__ __forceinline__ double av(int i, const double*) const { return ax[i]; }
  __device__ __forceinline__ void colsum(XlShared& sh, const double* v, bool p1) const { xl_colsum(sh, A, M, N, v, p1); }
  __device__ __forceinline__ void normal(XlShared& sh, const double* w, bool p1) const {
    __syncthreads();  // w was written by other threads
    xl_normal(sh, A, M, N, p1, w, H);
  }
  __device__ __forceinline__ bool factor(XlShared& sh, const double* w, bool p1) const {
    normal(sh, w, p1);
    return xl_cholesky(sh, H, N + (p1 ? 1 : 0), kLgPivot, true);
  }
  __device__ __forceinline__ bool full_rank(XlShared& sh, const double* w) const {
    normal(sh, w, false);
    return xl_cholesky(sh, H, N, 1e-12, false);
  }
  __device__ __forceinline__ void solve(XlShared& sh, int n, double* v) const { xl_solve(sh, H, n, v); }
  __device__ __forceinline__ double h_at(const XlShared&, int i, int j) const { return H[(size_t)i * kXlLD + j]; }
};

#ifndef QT_LP_PRIMITIVES_ONLY  // qt_lp_pieces.hip takes the primitives without the kernel (one definition per library)
// grid: persistent workgroups over the R * O programs; ws: gridDim.x * LpXl::ws_doubles(M) doubles
__global__ void __launch_bounds__(kLpNT) k_lp_ineq_xl(const double* __restrict__ A, int M, int N,
                                                      const double* __restrict__ C, int O, const double* __restrict__ bb,
                                                      int R, double* __restrict__ obj, double* __restrict__ xout,
                                                      int32_t* __restrict__ status, int32_t* __restrict__ iters,
                                                      double* __restrict__ ws) {
  __shared__ XlShared sh;
  lp_run(sh, LpXl(A, M, N, ws + blockIdx.x * LpXl::ws_doubles(M)), C, O, bb, R, obj, xout, status, iters);
}
#endif

}  // namespace qt
