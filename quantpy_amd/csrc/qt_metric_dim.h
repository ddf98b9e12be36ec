// Trace distance, infidelity and the Hermitian PSD root of DIM x DIM matrices, DIM = 16 / 32 (four- and five-qubit states,
// the Choi matrix of a two-qubit channel): geometry.py:23-56 for Hermitian arguments.
//
// The mapping of Small<NQ>::trace_dist / infidelity / psd_sqrt (qt_small.h) one level up, as qt_large.h has it for the
// estimators: one workgroup per trial, thread t = matrix element (i, j) = (t / DIM, t % DIM), two LDS images of pitch
// DIM + 1, __syncthreads() where the lane-group form has wave_sync(), and a two-level (DPP + LDS) reduction in a fixed order
// where it has the DPP butterfly.  The arithmetic per element is that of qt_small.h, operand for operand.
//
// Two things differ from the lane-group form:
//   * The sweeps are capped at 32 instead of 20 (kSweepCap): the rank-deficient S R S matrices of the infidelity need up to
//     24 at DIM = 32 in a model of this ordering.
//   * Every `break` is taken on a value that bsum() hands to all threads of the workgroup with the same bits, so a
//     barrier is never reached by part of a workgroup.  There is no other early exit.
#pragma once
#include <hip/hip_runtime.h>

#include "qt_args.h"   // centre_of
#include "qt_small.h"  // Metric
#include "qt_wave.h"

namespace qt {

template <int DIM>
struct MetricDim {
  static_assert(DIM == 16 || DIM == 32, "one thread per element: 256 or 1024 threads");
  static constexpr int d = DIM;
  static constexpr int NE = d * d;   // elements = threads per workgroup
  static constexpr int NT = NE;
  static constexpr int NW = NT / 64;
  static constexpr int LD = d + 1;            // row pitch of an image (qt_large.h: d leaves a d-way bank conflict on columns)
  static constexpr int MAT = 2 * LD * d;      // doubles per image; even, so both images are 16-byte aligned
  static constexpr int kSweepCap = 32;
  static constexpr int oRed = 2 * MAT;        // [16] partial sums of a reduction
  static constexpr int kDoubles = oRed + 16;  // static LDS per workgroup: 8.6 KB (DIM = 16), 33.1 KB (DIM = 32)

  struct Ctx {
    int t, i, j, e;  // thread, matrix element, its slot i * LD + j in an image
    double* sm;
    double tol2;
    __device__ __forceinline__ cd* A() const { return reinterpret_cast<cd*>(sm); }
    __device__ __forceinline__ cd* V() const { return reinterpret_cast<cd*>(sm + MAT); }
    __device__ __forceinline__ double* red() const { return sm + oRed; }
  };
  __device__ __forceinline__ static void make_ctx(Ctx& c, double* smem, double jtol2) {
    c.t = threadIdx.x;
    c.i = c.t / d;
    c.j = c.t % d;
    c.e = c.i * LD + c.j;
    c.sm = smem;
    c.tol2 = jtol2;
  }
  // The same context with the two images and the reduction slots wherever the caller has them: a kernel that holds more
  // in LDS than a metric (the n = 4, 5 chain of qt_mhmc_state_large.h) lends the scratch it already has.  A type of its own,
  // and every function below a template on the context: Ctx and the code of the kernels built on it stay what they were.
  struct CtxAt {
    int t, i, j, e;
    cd *a, *v;  // MAT doubles each
    double* r;  // [16]
    double tol2;
    __device__ __forceinline__ cd* A() const { return a; }
    __device__ __forceinline__ cd* V() const { return v; }
    __device__ __forceinline__ double* red() const { return r; }
  };
  __device__ __forceinline__ static void make_ctx(CtxAt& c, cd* img_a, cd* img_v, double* red, double jtol2) {
    c.t = threadIdx.x;
    c.i = c.t / d;
    c.j = c.t % d;
    c.e = c.i * LD + c.j;
    c.a = img_a;
    c.v = img_v;
    c.r = red;
    c.tol2 = jtol2;
  }

  // Sum over the workgroup, the same bits in every thread (Large::bsum): a wavefront's butterfly, then the NW partials in
  // a fixed order.  Two barriers: the first keeps the partials of the reduction before this one until everybody has read
  // them -- and orders any LDS image access before the call against any after it.
  template <class C>
  __device__ static double bsum(const C& c, double v) {
    v = gsum<64>(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) c.red()[threadIdx.x >> 6] = v;
    __syncthreads();
    if constexpr (NW == 16) {
      return gsum<16>(c.red()[threadIdx.x & 15]);
    } else {
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) s += c.red()[w];
      return s;
    }
  }
  __device__ __forceinline__ static double norm2(cd a) { return a.re * a.re + a.im * a.im; }
  __device__ __forceinline__ static double finite_or_nan(double n2, double val) {  // Small::finite_or_nan
    return n2 < __builtin_inf() ? val : __builtin_nan("");
  }

  // Small::jacobi_sweeps for one matrix per workgroup.  In: the thread's element of a Hermitian matrix A (real diagonal),
  // of V when VEC, and nrm = ||A||_F^2 as bsum gave it.  Out: A' = J^dagger A J with the eigenvalues on the diagonal,
  // V' = V J.  Round r = 1 .. d-1 rotates the d/2 disjoint pairs (k, k ^ r).  Left when off^2 <= tol2 * nrm (a NaN compares
  // false: such a matrix is never rotated), after kSweepCap sweeps at the latest.
  // VEC: a round publishes A and V, barrier, reads, barrier.  Without V the two images take the rounds in turn, one
  // barrier each: a thread that writes image p in round r + 2 has passed the barrier of round r + 1, which the slowest
  // thread reaches only after its reads of round r.  (The reduction at the head of a sweep, and of the caller behind the
  // loop, starts with a barrier.)
  template <bool VEC, class C>
  __device__ __forceinline__ static void sweeps(const C& c, cd& a_io, cd& v_io, double nrm) {
    cd a = a_io, v{0.0, 0.0};
    if constexpr (VEC) v = v_io;  // (without V the caller's object is neither read nor written: it folds away)
    const int i = c.i, j = c.j;
    cd* const Vi = c.V();
    int turn = 0;
    for (int sweep = 0; sweep < kSweepCap; ++sweep) {
      const double off = bsum(c, i != j ? norm2(a) : 0.0);
      if (!(off > c.tol2 * nrm)) break;  // workgroup-uniform: bsum's bits
#pragma unroll 1
      for (int r = 1; r < d; ++r) {
        cd* const Ai = (!VEC && turn) ? c.V() : c.A();
        Ai[c.e] = a;
        if constexpr (VEC) Vi[c.e] = v;
        __syncthreads();
        const int pj = j ^ r, pi = i ^ r;
        const int cp = j < pj ? j : pj, cq = j < pj ? pj : j;  // column pair, ordered
        const int rp = i < pi ? i : pi, rq = i < pi ? pi : i;  // row pair, ordered
        const double c_pp = Ai[cp * LD + cp].re, c_qq = Ai[cq * LD + cq].re;
        const cd c_pq = Ai[cp * LD + cq];
        const double r_pp = Ai[rp * LD + rp].re, r_qq = Ai[rq * LD + rq].re;
        const cd r_pq = Ai[rp * LD + rq];
        const cd a_c = Ai[i * LD + pj], a_r = Ai[pi * LD + j], a_x = Ai[pi * LD + pj];
        cd v_c{0.0, 0.0};
        if constexpr (VEC) {
          v_c = Vi[i * LD + pj];
          __syncthreads();  // all reads of these images are done before the next round overwrites them
        } else {
          turn ^= 1;
        }
        double cj, ci;
        cd wj, wi;
        rotation(c_pp, c_qq, c_pq, cj, wj);
        rotation(r_pp, r_qq, r_pq, ci, wi);
        if (j < pj) wj = cd{-wj.re, wj.im};  // J[pj][j]: -conj(w) if j is the lower index, else w
        if (i < pi) wi = cd{-wi.re, wi.im};
        // A'_ij = ci (a_ij cj + a_i,pj wj) + conj(wi) (a_pi,j cj + a_pi,pj wj) ;  V' = V J
        const cd t0 = cadd(cscale(a, cj), cmul(a_c, wj));
        const cd t1 = cadd(cscale(a_r, cj), cmul(a_x, wj));
        a = cadd(cscale(t0, ci), cmulc(t1, wi));
        if constexpr (VEC) v = cadd(cscale(v, cj), cmul(v_c, wj));
        if (i == j) a.im = 0.0;
      }
    }
    a_io = a;
    if constexpr (VEC) v_io = v;
  }

  // Small::trace_dist: sum_i |lambda_i(R - C)| / 2, the imaginary parts of the diagonal dropped; 0 below 1e-15.
  // In: the thread's elements of R and C.  Every thread returns the same bits.
  template <class C>
  __device__ static double trace_dist(const C& c, cd r, cd cen) {
    cd a{r.re - cen.re, c.i == c.j ? 0.0 : r.im - cen.im}, v{0.0, 0.0};
    const double n2 = bsum(c, norm2(a));
    sweeps<false>(c, a, v, n2);
    const double val = 0.5 * bsum(c, c.i == c.j ? fabs(a.re) : 0.0);
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }

  // Small::psd_sqrt: sum_k V_ik sqrt(max(lam_k, 0)) conj(V_jk), real on the diagonal; NaN throughout for a matrix that
  // holds a NaN or an infinity.
  template <class C>
  __device__ static cd psd_sqrt(const C& c, cd a) {
    const int i = c.i, j = c.j;
    cd* Ai = c.A();
    cd* Vi = c.V();
    cd v{i == j ? 1.0 : 0.0, 0.0};
    if (i == j) a.im = 0.0;
    const double n2 = bsum(c, norm2(a));
    sweeps<true>(c, a, v, n2);
    Ai[c.e] = a;  // (behind the barriers of the sweeps' last reduction)
    Vi[c.e] = v;
    __syncthreads();
    cd rr{0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < d; ++k) {
      const double lam = Ai[k * LD + k].re;
      const double w = sqrt(lam > 0.0 ? lam : 0.0);
      const cd p = cmulc(Vi[i * LD + k], Vi[j * LD + k]);
      rr.re += w * p.re;
      rr.im += w * p.im;
    }
    if (i == j) rr.im = 0.0;
    return cd{finite_or_nan(n2, rr.re), finite_or_nan(n2, rr.im)};
  }

  // Small::infidelity: 1 - (sum_i sqrt(max(mu_i, 0)))^2, mu the eigenvalues of the Hermitian part (real diagonal) of
  // M = S R S; 0 below 1e-15, small negatives included.  In: the thread's elements of R and of S = psd_sqrt(C).
  template <class C>
  __device__ static double infidelity(const C& c, cd r, cd s) {
    const int i = c.i, j = c.j;
    cd* X = c.A();
    cd* Y = c.V();
    X[c.e] = s;
    Y[c.e] = r;
    __syncthreads();
    cd t{0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < d; ++k) t = cadd(t, cmul(X[i * LD + k], Y[k * LD + j]));  // T = S R
    __syncthreads();
    Y[c.e] = t;
    __syncthreads();
    cd m{0.0, 0.0};
#pragma unroll 8
    for (int k = 0; k < d; ++k) m = cadd(m, cmul(Y[i * LD + k], X[k * LD + j]));  // M = T S
    __syncthreads();
    Y[c.e] = m;
    __syncthreads();
    const cd mt = Y[j * LD + i];
    cd a{0.5 * (m.re + mt.re), i == j ? 0.0 : 0.5 * (m.im - mt.im)}, v{0.0, 0.0};
    const double n2 = bsum(c, norm2(a));  // (its barriers: the read of Y above is done before the sweeps write)
    sweeps<false>(c, a, v, n2);
    const double rf = bsum(c, i == j ? sqrt(a.re > 0.0 ? a.re : 0.0) : 0.0);
    const double val = 1.0 - rf * rf;
    return finite_or_nan(n2, val < 1e-15 ? 0.0 : val);
  }
};

// roots[g] = the Hermitian root of centres[g], g = the workgroup (grid = G): the set-up launch of the infidelity
template <int DIM>
__global__ void __launch_bounds__(DIM* DIM) k_psd_sqrt_dim(const double* __restrict__ centres, int G, double jtol2,
                                                           double* __restrict__ roots) {
  using W = MetricDim<DIM>;
  __shared__ __attribute__((aligned(16))) double smem[W::kDoubles];
  typename W::Ctx c;
  W::make_ctx(c, smem, jtol2);
  const int g = blockIdx.x;
  if (g >= G) return;  // (workgroup-uniform, before any barrier)
  const size_t at = ((size_t)g * W::NE + c.t) * 2;
  const cd s = W::psd_sqrt(c, cd{centres[at], centres[at + 1]});
  roots[at] = s.re;
  roots[at + 1] = s.im;
}

// dist[b] = METRIC(rho[b], centre (g0 + b) % G), b = the workgroup (grid = B).  `centres`: the centres themselves (trace
// distance) or their roots as k_psd_sqrt_dim left them (infidelity).  A trial's bits depend on its two matrices alone.
template <int DIM, int METRIC>
__global__ void __launch_bounds__(DIM* DIM) k_metric_dist_dim(const double* __restrict__ rho, int B,
                                                              const double* __restrict__ centres, int G, int g0,
                                                              double jtol2, double* __restrict__ dist) {
  using W = MetricDim<DIM>;
  __shared__ __attribute__((aligned(16))) double smem[W::kDoubles];
  typename W::Ctx c;
  W::make_ctx(c, smem, jtol2);
  const int b = blockIdx.x;
  if (b >= B) return;  // (workgroup-uniform, before any barrier)
  const double* in = rho + ((size_t)b * W::NE + c.t) * 2;
  const double* cen = centre_of(centres, G, g0, b, 2 * W::NE) + 2 * c.t;
  const cd r{in[0], in[1]}, q{cen[0], cen[1]};
  const double v = METRIC == kMetricTrace ? W::trace_dist(c, r, q) : W::infidelity(c, r, q);
  if (c.t == 0) dist[b] = v;
}

}  // namespace qt
