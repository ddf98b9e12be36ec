// qt_lp.h -- a batch of small dense linear programs that share one constraint matrix (qt_lp_ineq_batch):
//
//     for r < R, o < O:  minimise C[o] . x  subject to  A x <= b[r],  x in R^N free   (N <= 64, any M >= N)
//
// The reference's PolytopeStateInterval (quantpy/tomography/interval.py:268-335) poses 2 * n_points of them, one
// cvxopt `solvers.lp` call each; all share A (the scaled POVM matrix) and differ in b (frequencies + delta) and in the
// sign of c.  One workgroup solves one LP at a time (persistent over the batch):
//
//   primal-dual interior point, Mehrotra predictor-corrector, on  A y + s = b, s > 0,  A^T z + c = 0, z > 0.
//   Newton system reduced to the normal matrix H = A^T diag(z / s) A (n x n, n <= 65), Cholesky in LDS.
//   Phase 1: the same iteration on  min t  s.t.  A x - t 1 <= b  (n = N + 1) from x = 0, t = max(-b, 0) + 1, which is
//   strictly feasible; it stops at the first iterate whose x alone is strictly feasible (min(b - A x) > 0).  If phase 1
//   converges instead (t* >= 0) the LP is infeasible.  Phase 2 starts from that x with z = mean(s) / s.
//
// A is read from global memory (L2: every workgroup reads the same A) in row blocks of kLpRB rows, so M is limited only
// by the workspace (six M-vectors per workgroup: s, z, r_p and three temporaries, in global memory).  Every loop has a
// bound: at most kLpCap iterations per phase, Cholesky and the row passes over fixed ranges.  Every branch that
// contains a barrier depends only on values that are uniform over the workgroup (block reductions, LDS).
//
// The iteration (lp_phase) and the per-workgroup driver (lp_run) are templates: k_lp_ineq_large (qt_lp_large.h, up to
// 255 variables) and k_lp_ineq_xl (qt_lp_xl.h, up to 1023) run the same text on their own primitives.  A kernel
// supplies one struct of primitives (LpSmall here).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace qt {

constexpr int kLpNT = 256;   // threads per workgroup (four wavefronts)
constexpr int kLpMaxN = 64;  // variables; phase 1 adds t
constexpr int kLpLD = 66;    // LDS row stride of the normal matrix (n <= 65)
constexpr int kLpRB = 32;    // rows of A per LDS block while forming H
constexpr int kLpCap = 100;  // iterations per phase

enum { LP_OPTIMAL = 0, LP_INFEASIBLE = 1, LP_UNBOUNDED = 2, LP_NOT_CONVERGED = 3, LP_FEASIBLE = 4 /* phase 1 only */ };

struct LpShared {
  double H[(kLpMaxN + 1) * kLpLD];
  double Ablk[kLpRB * kLpMaxN];
  double dblk[kLpRB];
  double y[kLpLD], dy[kLpLD], rd[kLpLD], u[kLpLD], c[kLpLD], diag[kLpLD];
  double part[4][kLpMaxN];
  double part_t[4];
  double red[4 * 4];
};

// Sum (or max) of K values over the workgroup; every thread gets the same bits (butterfly in the wavefront, the four
// wavefront results in a fixed order).
template <int K, bool MAX>
__device__ inline void lp_reduce(double (&v)[K], double* red) {
  for (int k = 0; k < K; ++k)
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v[k], off, 64);
      v[k] = MAX ? fmax(v[k], o) : v[k] + o;
    }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0)
    for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
  __syncthreads();
  for (int k = 0; k < K; ++k)
    v[k] = MAX ? fmax(fmax(red[k], red[K + k]), fmax(red[2 * K + k], red[3 * K + k]))
               : (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

// a_i . y over the first N columns (the caller adds the phase-1 column, which is -1 in every row)
__device__ inline double lp_row_dot(const double* __restrict__ a, int N, const double* y) {
  double acc = 0.0;
  for (int j = 0; j < N; ++j) acc = fma(a[j], y[j], acc);
  return acc;
}

// sh.u[j] = sum_i A[i][j] v[i] (j < N), sh.u[N] = sum_i v[i]; v is global, written by other threads before the call
__device__ inline void lp_colsum(LpShared& sh, const double* __restrict__ A, int M, int N, const double* v) {
  __syncthreads();
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  double acc = 0.0, tot = 0.0;
  for (int i = g; i < M; i += 4) {
    const double vi = v[i];
    if (j < N) acc = fma(A[(size_t)i * N + j], vi, acc);
    tot += vi;
  }
  sh.part[g][j] = acc;
  if (j == 0) sh.part_t[g] = tot;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < N) sh.u[t] = (sh.part[0][t] + sh.part[1][t]) + (sh.part[2][t] + sh.part[3][t]);
  if (t == 64) sh.u[N] = (sh.part_t[0] + sh.part_t[1]) + (sh.part_t[2] + sh.part_t[3]);
  __syncthreads();
}

// H = A^T diag(w) A for the first N columns, register-tiled 4 x 4 per thread over LDS row blocks of A
__device__ __noinline__ void lp_normal(LpShared& sh, const double* __restrict__ A, int M, int N, const double* w) {
  const int t = threadIdx.x, tj = t >> 4, tk = t & 15;
  double acc[4][4] = {};
  for (int r0 = 0; r0 < M; r0 += kLpRB) {
    __syncthreads();
    for (int e = t; e < kLpRB * kLpMaxN; e += kLpNT) {
      const int r = e / kLpMaxN, j = e % kLpMaxN, i = r0 + r;
      sh.Ablk[e] = (i < M && j < N) ? A[(size_t)i * N + j] : 0.0;
    }
    if (t < kLpRB) sh.dblk[t] = (r0 + t < M) ? w[r0 + t] : 0.0;
    __syncthreads();
    for (int r = 0; r < kLpRB; ++r) {
      const double* row = sh.Ablk + r * kLpMaxN;
      const double dr = sh.dblk[r];
      double p[4], q[4];
      for (int a = 0; a < 4; ++a) p[a] = dr * row[4 * tj + a];
      for (int b = 0; b < 4; ++b) q[b] = row[4 * tk + b];
      for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(p[a], q[b], acc[a][b]);
    }
  }
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) {
      const int i = 4 * tj + a, j = 4 * tk + b;
      if (i < N && j < N) sh.H[i * kLpLD + j] = acc[a][b];
    }
  __syncthreads();
}

// In-place Cholesky of the lower triangle of sh.H (n x n).  A pivot that is not finite or not above rel * (its
// diagonal entry before the factorisation) is a breakdown: returns false (the same answer in every thread).
__device__ inline bool lp_cholesky(LpShared& sh, int n, double rel) {
  const int t = threadIdx.x;
  if (t < n) sh.diag[t] = sh.H[t * kLpLD + t];
  __syncthreads();
  for (int k = 0; k < n; ++k) {
    const double p = sh.H[k * kLpLD + k];
    if (!(p > rel * sh.diag[k]) || !(p > 0.0) || !isfinite(p)) return false;
    const double l = sqrt(p);
    __syncthreads();  // every thread has read the pivot
    for (int i = k + t; i < n; i += kLpNT) sh.H[i * kLpLD + k] = (i == k) ? l : sh.H[i * kLpLD + k] / l;
    __syncthreads();
    const int m = n - k - 1;
    for (int e = t; e < m * m; e += kLpNT) {
      const int i = k + 1 + e / m, j = k + 1 + e % m;
      if (j <= i) sh.H[i * kLpLD + j] = fma(-sh.H[i * kLpLD + k], sh.H[j * kLpLD + k], sh.H[i * kLpLD + j]);
    }
    __syncthreads();
  }
  return true;
}

// v <- (L L^T)^{-1} v for the factor in sh.H
__device__ inline void lp_solve(LpShared& sh, int n, double* v) {
  const int t = threadIdx.x;
  for (int k = 0; k < n; ++k) {
    if (t == 0) v[k] /= sh.H[k * kLpLD + k];
    __syncthreads();
    for (int i = k + 1 + t; i < n; i += kLpNT) v[i] = fma(-sh.H[i * kLpLD + k], v[k], v[i]);
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    if (t == 0) v[k] /= sh.H[k * kLpLD + k];
    __syncthreads();
    for (int i = t; i < k; i += kLpNT) v[i] = fma(-sh.H[k * kLpLD + i], v[k], v[i]);
    __syncthreads();
  }
}

// Largest step in (0, inf) that keeps x + a dx >= 0 over this thread's rows, folded into *amax (kept as a minimum).
__device__ inline void lp_ratio(double x, double dx, double* amin) {
  if (dx < 0.0) *amin = fmin(*amin, -x / dx);
}

// What differs between the kernels that run lp_phase / lp_run below is one struct P per kernel.  It holds A, M, N and
// vec (the six M-vectors s, z, r_p, w, w2, w3 of this workgroup's workspace), names the kernel's LDS block (Shared: y,
// dy, rd, u, c, red and what the primitives need) and supplies
//   kCols                 the most columns it takes, the phase-1 column included (see QT_LP_COLS),
//   ws_doubles(M)         doubles of global workspace per workgroup,
//   matvec(v), av(i, v)   make A v available / (A v)_i for the v of the last matvec, over the first N columns,
//   colsum(sh, v, p1)     sh.u[j] = (A^T v)_j, and sh.u[N] = sum v (read in phase 1 only),
//   normal(sh, w, p1)     H = A^T diag(w) A with the phase-1 border, lower triangle (factor and full_rank start with it),
//   h_at(sh, i, j)        entry (i, j), j <= i, of H or of its factor, whichever came last (read by k_lp_pieces only),
//   factor(sh, w, p1)     H = A^T diag(w) A with the phase-1 border, then its Cholesky factor; false on a breakdown,
//   full_rank(sh, w)      the same for the rank test: no border, a pivot below 1e-12 of its diagonal entry is a breakdown,
//   solve(sh, n, v)       v <- H^{-1} v with the last factor.
// The LDS block is an argument of its own, from the kernel down, and not a member: the compiler then knows in every
// primitive that it is LDS, also in the ones it keeps as functions.  The members are forced inline (the struct never
// exists in memory), and so are lp_phase and lp_run; lp_normal, lg_normal and lg_solve are kept out of line, which is
// what the inliner chose before it was told: their register tiles are not live across the iteration.
// k_lp_ineq's: the normal matrix in LDS, (A v)_i computed where it is read (no M-vector for it).
struct LpSmall {
  using Shared = LpShared;
  static constexpr int kCols = kLpMaxN + 1;
  const double* __restrict__ A;
  int M, N;
  double* vec;

  __host__ __device__ static size_t ws_doubles(int M) { return (size_t)6 * M; }
  __device__ LpSmall(const double* A, int M, int N, double* ws) : A(A), M(M), N(N), vec(ws) {}
  __device__ __forceinline__ void matvec(const double*) const {}
  __device__ __forceinline__ double av(int i, const double* v) const { return lp_row_dot(A + (size_t)i * N, N, v); }
  __device__ __forceinline__ void colsum(LpShared& sh, const double* v, bool) const { lp_colsum(sh, A, M, N, v); }
  __device__ __forceinline__ void normal(LpShared& sh, const double* w, bool p1) const {
    const int t = threadIdx.x;
    __syncthreads();  // w was written by other threads
    lp_normal(sh, A, M, N, w);
    if (p1) {
      lp_colsum(sh, A, M, N, w);
      if (t < N) sh.H[N * kLpLD + t] = -sh.u[t];
      if (t == 64) sh.H[N * kLpLD + N] = sh.u[N];
      __syncthreads();
    }
  }
  __device__ __forceinline__ bool factor(LpShared& sh, const double* w, bool p1) const {
    normal(sh, w, p1);
    return lp_cholesky(sh, N + (p1 ? 1 : 0), 0.0);
  }
  __device__ __forceinline__ bool full_rank(LpShared& sh, const double* w) const {
    normal(sh, w, false);
    return lp_cholesky(sh, N, 1e-12);
  }
  __device__ __forceinline__ void solve(LpShared& sh, int n, double* v) const { lp_solve(sh, n, v); }
  // entry (i, j), j <= i, of the normal matrix or of its factor, whichever was computed last (k_lp_pieces reads them out)
  __device__ __forceinline__ double h_at(const LpShared& sh, int i, int j) const { return sh.H[i * kLpLD + j]; }
};

// QT_LP_COLS(P, j, n, statement): the statement for every column j < n, spread over the workgroup.  Where P's columns fit
// its threads (kCols <= kLpNT, the two kernels with up to 256 columns) that is `if (t < n)`, spelled as it was before
// there was a third kernel (their device code is compared, scripts/isa_identity.py); otherwise a loop in strides of the
// workgroup.  A macro and not a function that takes a lambda: the captures change the code of the first two kernels.
#define QT_LP_COLS(P, j, n, ...)                     \
  if constexpr (P::kCols <= kLpNT) {                 \
    const int j = threadIdx.x;                       \
    if (j < (n)) __VA_ARGS__                         \
  } else {                                           \
    for (int j = threadIdx.x; j < (n); j += kLpNT) __VA_ARGS__ \
  }

// One phase of the interior-point method, for every kernel: every tolerance and test of the method is here and in
// lp_run, nowhere else in device code.  In: sh.y[0..n) (n = N + p1), sh.c[0..n), s, z (global, this LP's rows).
// Returns LP_FEASIBLE (phase 1: x strictly feasible), LP_INFEASIBLE (phase 1 converged), LP_OPTIMAL, LP_UNBOUNDED or
// LP_NOT_CONVERGED.  On LP_FEASIBLE the last matvec was of sh.y.
template <class P>
__device__ __forceinline__ int lp_phase(typename P::Shared& sh, const P& p, bool p1, const double* __restrict__ b, double amax, double bn, double cn, int* iters) {
  constexpr double kTol = 1e-10;
  const int t = threadIdx.x, M = p.M, N = p.N, n = N + (p1 ? 1 : 0);
  double *s = p.vec, *z = s + M, *rp = z + M, *w = rp + M, *w2 = w + M, *w3 = w2 + M;
  for (int it = 0; it < kLpCap; ++it) {
    // ---- residuals and stopping tests
    p.matvec(sh.y);
    double sums[2] = {0.0, 0.0}, maxs[2] = {0.0, -INFINITY};  // s.z, sum z | max|r_p|, max(A x - b)
    for (int i = t; i < M; i += kLpNT) {
      const double ax = p.av(i, sh.y);  // phase 2 starts from s = b - ax, bit for bit
      const double r = (p1 ? ax - sh.y[N] : ax) + s[i] - b[i];
      rp[i] = r;
      sums[0] = fma(s[i], z[i], sums[0]);
      sums[1] += z[i];
      maxs[0] = fmax(maxs[0], fabs(r));
      maxs[1] = fmax(maxs[1], ax - b[i]);
    }
    lp_reduce<2, false>(sums, sh.red);
    lp_reduce<2, true>(maxs, sh.red);
    p.colsum(sh, z, p1);
    double ynorm = 0.0, pobj = 0.0, dres = 0.0;
    for (int j = 0; j < n; ++j) {
      ynorm += fabs(sh.y[j]);
      pobj = fma(sh.c[j], sh.y[j], pobj);
      const double rdj = (j < N ? sh.u[j] : -sh.u[N]) + sh.c[j];
      dres = fmax(dres, fabs(rdj));
    }
    __syncthreads();
    QT_LP_COLS(P, j, n, sh.rd[j] = (j < N ? sh.u[j] : -sh.u[N]) + sh.c[j];)
    __syncthreads();
    *iters += 1;
    const double gap = sums[0], mu = gap / M;
    const double pres = maxs[0] / fmax(bn, amax * ynorm), dres_s = dres / fmax(cn, amax * sums[1]);
    if (!isfinite(gap) || !isfinite(pres) || !isfinite(dres_s) || !isfinite(pobj)) return LP_NOT_CONVERGED;
    if (p1 && maxs[1] < 0.0) return LP_FEASIBLE;
    if (pres <= kTol && dres_s <= kTol && gap <= kTol * fmax(1.0, fabs(pobj))) return p1 ? LP_INFEASIBLE : LP_OPTIMAL;
    // phase 1: c.y - s.z is the dual objective up to the residuals, a lower bound on t*; once it is positive the
    // multipliers certify infeasibility (Farkas), before the degenerate phase-1 optimum makes H singular
    if (p1 && pres <= kTol && dres_s <= kTol && pobj - gap > 1e-9 * fmax(1.0, fabs(pobj))) return LP_INFEASIBLE;
    if (!p1 && pres <= 1e-8 && pobj < -1e10 * cn * bn) return LP_UNBOUNDED;

    // ---- normal matrix and its factor
    for (int i = t; i < M; i += kLpNT) w[i] = z[i] / s[i];
    if (!p.factor(sh, w, p1)) return LP_NOT_CONVERGED;

    // ---- predictor: r_sz = s z
    for (int i = t; i < M; i += kLpNT) w[i] = z[i] - z[i] * rp[i] / s[i];
    p.colsum(sh, w, p1);
    QT_LP_COLS(P, j, n, sh.dy[j] = -sh.rd[j] + (j < N ? sh.u[j] : -sh.u[N]);)
    __syncthreads();
    p.solve(sh, n, sh.dy);
    p.matvec(sh.dy);
    double al[2] = {-1.0, -1.0};  // -(largest primal / dual step), as a max
    {
      double ap = INFINITY, ad = INFINITY;
      for (int i = t; i < M; i += kLpNT) {
        const double ady = p.av(i, sh.dy);
        const double ds = -rp[i] - (p1 ? ady - sh.dy[N] : ady);
        const double dz = -z[i] - z[i] * ds / s[i];
        w2[i] = ds;
        w3[i] = dz;
        lp_ratio(s[i], ds, &ap);
        lp_ratio(z[i], dz, &ad);
      }
      al[0] = -fmin(1.0, ap);
      al[1] = -fmin(1.0, ad);
    }
    lp_reduce<2, true>(al, sh.red);
    double muaff[1] = {0.0};
    for (int i = t; i < M; i += kLpNT) muaff[0] = fma(s[i] - al[0] * w2[i], z[i] - al[1] * w3[i], muaff[0]);
    lp_reduce<1, false>(muaff, sh.red);
    const double ratio = muaff[0] / M / mu, sigma_mu = ratio * ratio * ratio * mu;

    // ---- corrector: r_sz = s z + ds_aff dz_aff - sigma mu  (kept in w2)
    for (int i = t; i < M; i += kLpNT) {
      const double rsz = s[i] * z[i] + w2[i] * w3[i] - sigma_mu;
      w2[i] = rsz;
      w[i] = (rsz - z[i] * rp[i]) / s[i];
    }
    p.colsum(sh, w, p1);
    QT_LP_COLS(P, j, n, sh.dy[j] = -sh.rd[j] + (j < N ? sh.u[j] : -sh.u[N]);)
    __syncthreads();
    p.solve(sh, n, sh.dy);
    p.matvec(sh.dy);
    {
      double ap = INFINITY, ad = INFINITY;
      for (int i = t; i < M; i += kLpNT) {
        const double ady = p.av(i, sh.dy);
        const double ds = -rp[i] - (p1 ? ady - sh.dy[N] : ady);
        const double dz = (-w2[i] - z[i] * ds) / s[i];
        rp[i] = ds;
        w3[i] = dz;
        lp_ratio(s[i], ds, &ap);
        lp_ratio(z[i], dz, &ad);
      }
      al[0] = -ap;
      al[1] = -ad;
    }
    lp_reduce<2, true>(al, sh.red);
    const double ap = fmin(1.0, -0.99 * al[0]), ad = fmin(1.0, -0.99 * al[1]);
    for (int i = t; i < M; i += kLpNT) {
      s[i] = fma(ap, rp[i], s[i]);
      z[i] = fma(ad, w3[i], z[i]);
    }
    QT_LP_COLS(P, j, n, sh.y[j] = fma(ap, sh.dy[j], sh.y[j]);)
    __syncthreads();
  }
  return LP_NOT_CONVERGED;
}

// One workgroup of either kernel, persistent over the R * O programs: rank test, then for every program the phase-1
// start, the hand-over to phase 2 and the write-out.
template <class P>
__device__ __forceinline__ void lp_run(typename P::Shared& sh, const P& p, const double* __restrict__ C, int O, const double* __restrict__ bb, int R,
                       double* __restrict__ obj, double* __restrict__ xout, int32_t* __restrict__ status,
                       int32_t* __restrict__ iters) {
  const int t = threadIdx.x, M = p.M, N = p.N;
  const double* __restrict__ A = p.A;
  double *s = p.vec, *z = s + M, *w = z + 2 * M;
  // max |A|: the scale of the rounding in A y and A^T z
  double amax[1] = {0.0};
  for (size_t e = t; e < (size_t)M * N; e += kLpNT) amax[0] = fmax(amax[0], fabs(A[e]));
  lp_reduce<1, true>(amax, sh.red);
  // rank test, once: a pivot of the Cholesky factor of A^T A below 1e-12 of its diagonal entry (cond(A) above ~1e6)
  // is a breakdown, and every program of the batch reports NOT_CONVERGED (no pivot is replaced here: that would hide it)
  for (int i = t; i < M; i += kLpNT) w[i] = 1.0;
  const bool full_rank = p.full_rank(sh, w);
  for (int lp = blockIdx.x; lp < R * O; lp += gridDim.x) {
    const int r = lp / O, o = lp % O;
    const double* b = bb + (size_t)r * M;
    const double* c = C + (size_t)o * N;
    double bm[2] = {0.0, -INFINITY};  // max |b|, max(-b)
    for (int i = t; i < M; i += kLpNT) {
      bm[0] = fmax(bm[0], fabs(b[i]));
      bm[1] = fmax(bm[1], -b[i]);
    }
    lp_reduce<2, true>(bm, sh.red);
    const double bn = fmax(1.0, bm[0]);
    int it = 0;
    int st = LP_NOT_CONVERGED;
    // phase 1 from x = 0, t0 = max(-b, 0) + 1: s = b + t0 >= 1, z = 1 / M (the dual's sum z = 1 holds)
    const double t0 = fmax(bm[1], 0.0) + 1.0;
    QT_LP_COLS(P, j, N + 1, {
      sh.y[j] = (j == N) ? t0 : 0.0;
      sh.c[j] = (j == N) ? 1.0 : 0.0;
    })
    for (int i = t; i < M; i += kLpNT) {
      s[i] = b[i] + t0;
      z[i] = 1.0 / M;
    }
    __syncthreads();
    if (full_rank) st = lp_phase(sh, p, true, b, amax[0], bn, 1.0, &it);
    if (st == LP_FEASIBLE) {
      // phase 2 from the strictly feasible x: s = b - A x (the A x of phase 1's last matvec), z = mean(s) / s
      double cm[1] = {0.0}, ssum[1] = {0.0};
      for (int j = t; j < N; j += kLpNT) cm[0] = fmax(cm[0], fabs(c[j]));
      for (int i = t; i < M; i += kLpNT) {
        s[i] = b[i] - p.av(i, sh.y);
        ssum[0] += s[i];
      }
      lp_reduce<1, true>(cm, sh.red);
      lp_reduce<1, false>(ssum, sh.red);
      const double smean = ssum[0] / M;
      for (int i = t; i < M; i += kLpNT) z[i] = smean / s[i];
      QT_LP_COLS(P, j, N, sh.c[j] = c[j];)
      __syncthreads();
      st = lp_phase(sh, p, false, b, amax[0], bn, fmax(1.0, cm[0]), &it);
    }
    if (t == 0) {
      double val = NAN;
      if (st == LP_OPTIMAL) {
        val = 0.0;
        for (int j = 0; j < N; ++j) val = fma(c[j], sh.y[j], val);
      } else if (st == LP_INFEASIBLE) {
        val = INFINITY;
      } else if (st == LP_UNBOUNDED) {
        val = -INFINITY;
      }
      obj[lp] = val;
      status[lp] = st;
      if (iters) iters[lp] = it;
    }
    if (xout) {
      QT_LP_COLS(P, j, N, xout[(size_t)lp * N + j] = sh.y[j];)
    }
    __syncthreads();  // sh.y / sh.c are rewritten by the next program
  }
}

#undef QT_LP_COLS

#ifndef QT_LP_PRIMITIVES_ONLY  // qt_lp_pieces.hip takes the primitives without the kernel (one definition per library)
// grid: persistent workgroups over the R * O programs; ws: gridDim.x * LpSmall::ws_doubles(M) doubles
__global__ void __launch_bounds__(kLpNT) k_lp_ineq(const double* __restrict__ A, int M, int N,
                                                   const double* __restrict__ C, int O, const double* __restrict__ bb,
                                                   int R, double* __restrict__ obj, double* __restrict__ xout,
                                                   int32_t* __restrict__ status, int32_t* __restrict__ iters,
                                                   double* __restrict__ ws) {
  __shared__ LpShared sh;
  lp_run(sh, LpSmall(A, M, N, ws + blockIdx.x * LpSmall::ws_doubles(M)), C, O, bb, R, obj, xout, status, iters);
}
#endif

}  // namespace qt
