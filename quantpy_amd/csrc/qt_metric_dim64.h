// Trace distance, infidelity and the Hermitian PSD root of 64 x 64 matrices (the Choi matrix of a three-qubit channel, a
// six-qubit object): geometry.py:23-56 for Hermitian arguments, the functions of MetricDim<DIM> (qt_metric_dim.h) with four
// elements per thread.
//
// One workgroup of 1024 threads per trial.  Thread t holds row i = t / 16 and the columns j = t % 16 + 16 m, m = 0 .. 3:
// the sixteen lanes of a row read and write sixteen consecutive elements of an image (one 256-byte LDS row), and a
// wavefront covers four rows of every column.  The images have pitch 65, as those of MetricDim have pitch DIM + 1; the
// reduction is bsum's of DIM = 32 (sixteen wavefronts, a fixed order).
//
// What differs from MetricDim:
//   * A round's 32 rotations are formed ONCE, by 32 lanes of wavefront 0 from the published diagonal and pivot entries,
//     and handed to everybody through a 2 KB table in LDS (rot: per index k the c and the signed w of column k of J),
//     which costs one more barrier per round.  The one-thread-per-element form has every element form its two, an rsq,
//     an rcp and an rsqrt with their Newton steps apiece: at d = 64 that would be 8192 rotations per round for 32.
//   * The eigenvalue-only sweeps (trace distance, S R S) ping-pong the two images: two barriers per round (image, table).
//     The sweeps with eigenvectors (the root) hold A and V in the two images and take a third barrier per round, behind
//     the reads.  The table needs no second copy: it is written between a round's two barriers and read behind the
//     second, and the next write is behind the next round's first barrier, which every reader has then passed.
//   * LDS is dynamic, kLdsBytes = 135 296 B (two images of 66 560 B, 16 partial sums, the table): one workgroup per CU.
//   * The sweeps are capped at 48 instead of 32 (kSweepCap): a model of this ordering needs up to 29 for the root of a
//     PSD-clipped matrix and 27 for S R S.
// Every `break` is taken on a value that bsum() hands to all threads with the same bits; there is no other early exit.
#pragma once
#include <hip/hip_runtime.h>

#include "qt_args.h"   // centre_of
#include "qt_small.h"  // Metric
#include "qt_wave.h"

namespace qt {

struct MetricDim64 {
  static constexpr int d = 64;
  static constexpr int NE = d * d;
  static constexpr int NT = 1024;
  static constexpr int EPT = NE / NT;        // elements per thread
  static constexpr int CS = d / EPT;         // column stride between a thread's elements = lanes per row
  static constexpr int NW = NT / 64;
  static constexpr int LD = d + 1;           // row pitch of an image
  static constexpr int MAT = 2 * LD * d;     // doubles per image; even, so both images are 16-byte aligned
  static constexpr int kSweepCap = 48;
  static constexpr int oRed = 2 * MAT;       // [16] partial sums of a reduction
  static constexpr int oRot = oRed + 16;     // [d][4]: c, w.re, w.im of column k of the round's J (32-byte entries)
  static constexpr int kDoubles = oRot + 4 * d;
  static constexpr size_t kLdsBytes = kDoubles * sizeof(double);
  static_assert(NW == 16 && EPT == 4 && oRot % 2 == 0, "bsum's second level is gsum<16>; cd arrays start at even offsets");

  struct Ctx {
    int t, i, j0, e0;  // thread, its row, its first column, the slot i * LD + j0 of its first element in an image
    double* sm;
    double tol2;
    __device__ __forceinline__ cd* A() const { return reinterpret_cast<cd*>(sm); }
    __device__ __forceinline__ cd* V() const { return reinterpret_cast<cd*>(sm + MAT); }
    __device__ __forceinline__ double* red() const { return sm + oRed; }
    __device__ __forceinline__ double* rot() const { return sm + oRot; }
  };
  __device__ __forceinline__ static void make_ctx(Ctx& c, double* smem, double jtol2) {
    c.t = threadIdx.x;
    c.i = c.t / CS;
    c.j0 = c.t % CS;
    c.e0 = c.i * LD + c.j0;
    c.sm = smem;
    c.tol2 = jtol2;
  }
  // The thread's elements of a [.][64][64][2] array, matrix `b`: 16 lanes read 256 consecutive bytes
  __device__ __forceinline__ static void load(const Ctx& c, const double* __restrict__ base, size_t b, cd (&x)[EPT]) {
    const double* p = base + (b * NE + (size_t)c.i * d + c.j0) * 2;
#pragma unroll
    for (int m = 0; m < EPT; ++m) x[m] = cd{p[2 * CS * m], p[2 * CS * m + 1]};
  }
  __device__ __forceinline__ static void put(const Ctx& c, cd* img, const cd (&x)[EPT]) {
#pragma unroll
    for (int m = 0; m < EPT; ++m) img[c.e0 + CS * m] = x[m];
  }

  // MetricDim<32>::bsum: a wavefront's butterfly, then the 16 partials in a fixed order; the same bits in every thread.
  // Two barriers, the first of which orders any LDS access before the call against any after it.
  __device__ static double bsum(const Ctx& c, double v) {
    v = gsum<64>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) c.red()[threadIdx.x >> 6] = v;
    __syncthreads();
    return gsum<16>(c.red()[threadIdx.x & 15]);
  }
  __device__ __forceinline__ static double norm2(cd a) { return a.re * a.re + a.im * a.im; }
  __device__ __forceinline__ static double finite_or_nan(double n2, double val) {
    return n2 < __builtin_inf() ? val : __builtin_nan("");
  }

  // MetricDim::sweeps with four elements per thread.  In: the thread's elements of a Hermitian matrix A (real diagonal),
  // of V when VEC, and nrm = ||A||_F^2 as bsum gave it.  Out: A' = J^dagger A J with the eigenvalues on the diagonal,
  // V' = V J.  Round r = 1 .. 63 rotates the 32 disjoint pairs (k, k ^ r).  Left when off^2 <= tol2 * nrm (a NaN compares
  // false: such a matrix is never rotated), after kSweepCap sweeps at the latest.
  template <bool VEC>
  __device__ __forceinline__ static void sweeps(const Ctx& c, cd (&a)[EPT], cd (&v)[EPT], double nrm) {
    const int i = c.i;
    cd* const Vi = c.V();
    double* const rot = c.rot();
    int turn = 0;
    for (int sweep = 0; sweep < kSweepCap; ++sweep) {
      double o = 0.0;
#pragma unroll
      for (int m = 0; m < EPT; ++m) o += i != c.j0 + CS * m ? norm2(a[m]) : 0.0;
      const double off = bsum(c, o);
      if (!(off > c.tol2 * nrm)) break;  // workgroup-uniform: bsum's bits
#pragma unroll 1
      for (int r = 1; r < d; ++r) {
        cd* const Ai = (!VEC && turn) ? c.V() : c.A();
        put(c, Ai, a);
        if constexpr (VEC) put(c, Vi, v);
        __syncthreads();
        if (c.t < d) {  // (wavefront 0, whole)
          const int p = c.t, q = c.t ^ r;
          if (p < q) {
            double cs;
            cd w;
            rotation(Ai[p * LD + p].re, Ai[q * LD + q].re, Ai[p * LD + q], cs, w);
            // column k of J: J[k ^ r][k] = -conj(w) if k is the lower index of its pair, else w
            rot[4 * p] = cs, rot[4 * p + 1] = -w.re, rot[4 * p + 2] = w.im;
            rot[4 * q] = cs, rot[4 * q + 1] = w.re, rot[4 * q + 2] = w.im;
          }
        }
        __syncthreads();
        const int pi = i ^ r;
        const double ci = rot[4 * i];
        const cd wi{rot[4 * i + 1], rot[4 * i + 2]};
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
          const int j = c.j0 + CS * m, pj = j ^ r;
          const double cj = rot[4 * j];
          const cd wj{rot[4 * j + 1], rot[4 * j + 2]};
          const cd a_c = Ai[i * LD + pj], a_r = Ai[pi * LD + j], a_x = Ai[pi * LD + pj];
          // A'_ij = ci (a_ij cj + a_i,pj wj) + conj(wi) (a_pi,j cj + a_pi,pj wj) ;  V' = V J
          const cd t0 = cadd(cscale(a[m], cj), cmul(a_c, wj));
          const cd t1 = cadd(cscale(a_r, cj), cmul(a_x, wj));
          a[m] = cadd(cscale(t0, ci), cmulc(t1, wi));
          if constexpr (VEC) v[m] = cadd(cscale(v[m], cj), cmul(Vi[i * LD + pj], wj));
          if (i == j) a[m].im = 0.0;
        }
        if constexpr (VEC)
          __syncthreads();  // all reads of the two images are done before the next round overwrites them
        else
          turn ^= 1;
      }
    }
  }

  // MetricDim::trace_dist: sum_i |lambda_i(R - C)| / 2, the imaginary parts of the diagonal dropped; 0 below 1e-15.
  // In: the thread's elements of R and C.  Every thread returns the same bits.
  __device__ static double trace_dist(const Ctx& c, const cd (&r)[EPT], const cd (&cen)[EPT]) {
    cd a[EPT], v[EPT];
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      a[m] = cd{r[m].re - cen[m].re, c.i == c.j0 + CS * m ? 0.0 : r[m].im - cen[m].im};
      s += norm2(a[m]);
    }
    const double n2 = bsum(c, s);
    sweeps<false>(c, a, v, n2);
    s = 0.0;
#pragma unroll
    for (int m = 0; m < EPT; ++m) s += c.i == c.j0 + CS * m ? fabs(a[m].re) : 0.0;
    const double val = 0.5 * bsum(c, s);
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }

  // MetricDim::psd_sqrt: sum_k V_ik sqrt(max(lam_k, 0)) conj(V_jk), real on the diagonal; NaN throughout for a matrix that
  // holds a NaN or an infinity.  In: the thread's elements, replaced by those of the root.
  __device__ static void psd_sqrt(const Ctx& c, cd (&a)[EPT]) {
    const int i = c.i;
    cd* Ai = c.A();
    cd* Vi = c.V();
    cd v[EPT];
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      const bool diag = i == c.j0 + CS * m;
      v[m] = cd{diag ? 1.0 : 0.0, 0.0};
      if (diag) a[m].im = 0.0;
      s += norm2(a[m]);
    }
    const double n2 = bsum(c, s);
    sweeps<true>(c, a, v, n2);
    put(c, Ai, a);  // (behind the barriers of the sweeps' last reduction)
    put(c, Vi, v);
    __syncthreads();
    cd rr[EPT];
#pragma unroll
    for (int m = 0; m < EPT; ++m) rr[m] = cd{0.0, 0.0};
#pragma unroll 2
    for (int k = 0; k < d; ++k) {
      const double lam = Ai[k * LD + k].re;
      const double w = sqrt(lam > 0.0 ? lam : 0.0);
      const cd vi = Vi[i * LD + k];
#pragma unroll
      for (int m = 0; m < EPT; ++m) {
        const cd p = cmulc(vi, Vi[(c.j0 + CS * m) * LD + k]);
        rr[m].re += w * p.re;
        rr[m].im += w * p.im;
      }
    }
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      if (i == c.j0 + CS * m) rr[m].im = 0.0;
      a[m] = cd{finite_or_nan(n2, rr[m].re), finite_or_nan(n2, rr[m].im)};
    }
  }

  // out = X Y for the two images as they stand (the thread's four elements of row i)
  __device__ __forceinline__ static void matmul(const Ctx& c, const cd* X, const cd* Y, cd (&out)[EPT]) {
#pragma unroll
    for (int m = 0; m < EPT; ++m) out[m] = cd{0.0, 0.0};
#pragma unroll 4
    for (int k = 0; k < d; ++k) {
      const cd x = X[c.i * LD + k];
#pragma unroll
      for (int m = 0; m < EPT; ++m) out[m] = cadd(out[m], cmul(x, Y[k * LD + c.j0 + CS * m]));
    }
  }

  // MetricDim::infidelity: 1 - (sum_i sqrt(max(mu_i, 0)))^2, mu the eigenvalues of the Hermitian part (real diagonal) of
  // M = S R S; 0 below 1e-15, small negatives included.  In: the thread's elements of R and of S = psd_sqrt(C).
  __device__ static double infidelity(const Ctx& c, const cd (&r)[EPT], const cd (&s)[EPT]) {
    const int i = c.i;
    cd* X = c.A();
    cd* Y = c.V();
    put(c, X, s);
    put(c, Y, r);
    __syncthreads();
    cd t[EPT], a[EPT], v[EPT];
    matmul(c, X, Y, t);  // T = S R
    __syncthreads();
    put(c, Y, t);
    __syncthreads();
    matmul(c, Y, X, t);  // M = T S
    __syncthreads();
    put(c, Y, t);
    __syncthreads();
    double n = 0.0;
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
      const int j = c.j0 + CS * m;
      const cd mt = Y[j * LD + i];
      a[m] = cd{0.5 * (t[m].re + mt.re), i == j ? 0.0 : 0.5 * (t[m].im - mt.im)};
      n += norm2(a[m]);
    }
    const double n2 = bsum(c, n);  // (its barriers: the read of Y above is done before the sweeps write)
    sweeps<false>(c, a, v, n2);
    n = 0.0;
#pragma unroll
    for (int m = 0; m < EPT; ++m) n += i == c.j0 + CS * m ? sqrt(a[m].re > 0.0 ? a[m].re : 0.0) : 0.0;
    const double rf = bsum(c, n);
    const double val = 1.0 - rf * rf;
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }
};

// roots[g] = the Hermitian root of centres[g], g = the workgroup (grid = G): the set-up launch of the infidelity.
// Dynamic LDS: MetricDim64::kLdsBytes.
__global__ void __launch_bounds__(MetricDim64::NT) k_psd_sqrt_dim64(const double* __restrict__ centres, int G, double jtol2,
                                                                    double* __restrict__ roots) {
  using W = MetricDim64;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  W::Ctx c;
  W::make_ctx(c, smem, jtol2);
  const int g = blockIdx.x;
  if (g >= G) return;  // (workgroup-uniform, before any barrier)
  cd a[W::EPT];
  W::load(c, centres, (size_t)g, a);
  W::psd_sqrt(c, a);
  double* out = roots + ((size_t)g * W::NE + (size_t)c.i * W::d + c.j0) * 2;
#pragma unroll
  for (int m = 0; m < W::EPT; ++m) {
    out[2 * W::CS * m] = a[m].re;
    out[2 * W::CS * m + 1] = a[m].im;
  }
}

// dist[b] = METRIC(rho[b], centre (g0 + b) % G), b = the workgroup (grid = B).  `centres`: the centres themselves (trace
// distance) or their roots as k_psd_sqrt_dim64 left them (infidelity).  A trial's bits depend on its two matrices alone.
// Dynamic LDS: MetricDim64::kLdsBytes.
template <int METRIC>
__global__ void __launch_bounds__(MetricDim64::NT) k_metric_dist_dim64(const double* __restrict__ rho, int B,
                                                                       const double* __restrict__ centres, int G, int g0,
                                                                       double jtol2, double* __restrict__ dist) {
  using W = MetricDim64;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  W::Ctx c;
  W::make_ctx(c, smem, jtol2);
  const int b = blockIdx.x;
  if (b >= B) return;  // (workgroup-uniform, before any barrier)
  cd r[W::EPT], q[W::EPT];
  W::load(c, rho, (size_t)b, r);
  W::load(c, centre_of(centres, G, g0, b, 2 * W::NE), 0, q);
  const double v = METRIC == kMetricTrace ? W::trace_dist(c, r, q) : W::infidelity(c, r, q);
  if (c.t == 0) dist[b] = v;
}

}  // namespace qt
