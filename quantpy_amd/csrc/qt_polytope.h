// qt_polytope.h -- the coverage study of the confidence polytope (Kiktenko et al., arXiv:2109.04734, Fig. 1; reference
// quantpy/tomography/polytopes/utils.py and verification.py) over a batch of simulated tomographies, FP64.
//
// A trial is a count table c[R][K] (R settings, K outcomes, shots[r] per setting), f = clip(c / shots[r], EPS, 1 - EPS).
//
//   confidence(delta) = prod_r max(1 - sum_k e[r][k], 0),   e = exp(-shots[r] KL(f || clip(f + delta, EPS, 1 - EPS))),
//                       e = 0 where the clip reached its top (KL = +inf) and where |f - 1| < 2 EPS      (utils.py:4-13)
//   delta(level)      = bisection on [1e-10, 1] down to a width of 1e-10, the left end moving while
//                       confidence(mid) < level + 1e-10; the last midpoint                               (utils.py:16-27)
//   hit(level)        = min over rows of (b - t) > -EPS,  b = clip(f + delta) (state) or f + delta (process),
//                       t = the true outcome probabilities                          (verification.py:33-34, :70-75)
//
// Two mappings, chosen by the host from the shape alone (never from the batch size, so a result does not depend on how
// the trials are split over calls):
//
//   wave teams  (R K <= 64, K a power of two): a team of TS = pow2 >= R K lanes owns one (trial, level) pair, one table
//               entry per lane, 64 / TS teams per wavefront; f, shots and t live in registers.  No LDS, no barrier.
//   workgroup   (every other shape): a workgroup of NT threads owns a trial and loops over its levels.  f is staged once
//               per trial in LDS (POLY_LDS) or, where R K doubles do not fit, recomputed from the counts in L2
//               (POLY_GLOBAL: no size limit).  G lanes (a power of two <= 64, chosen by the host) share a setting: each
//               sums the outcomes k = g, g + G, ... in order, a butterfly over the G lanes adds them.
//
// The sum over k and the product over r run in a fixed order: serial per lane, butterfly in the wavefront (both partners
// of an exchange compute the same commutative operation, so every lane ends with the same bits), wavefront partials in
// index order.  The bisection's comparison is therefore uniform over the team / workgroup, and every loop has a cap.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace qt {

constexpr double kPolyEps = 1e-15;
constexpr int kPolyCap = 64;  // bisection steps (34 are taken: the bracket halves whatever the data)

enum { POLY_LDS = 0, POLY_GLOBAL = 1 };

// lanes-per-setting layout of the workgroup mapping
struct PolyShape {
  int R, K;
  int G, gshift;  // lanes per setting, log2
};

__device__ inline double poly_freq(int64_t c, double n) { return fmin(fmax((double)c / n, kPolyEps), 1.0 - kPolyEps); }

// one entry's exp(-n KL), with the reference's two special cases
__device__ inline double poly_term(double f, double n, double delta) {
  const double s = fmin(fmax(f + delta, kPolyEps), 1.0 - kPolyEps);
  if (fabs(f - 1.0) < 2 * kPolyEps || !(s < 1.0 - kPolyEps)) return 0.0;
  const double g = 1.0 - f;
  const double kl = f * log(f / s) + g * log(g / (1.0 - s));
  return exp(-n * kl);
}

__device__ inline double poly_bound(double f, double delta, int clip_b) {
  const double b = f + delta;
  return clip_b ? fmin(fmax(b, kPolyEps), 1.0 - kPolyEps) : b;
}

// ---- wave teams -----------------------------------------------------------------------------------------------------
struct PolyTeam {
  double f, n, t;  // this lane's entry (inactive lanes: unused)
  bool active;
  int K, TS;
};

__device__ inline double poly_team_conf(const PolyTeam& m, double delta) {
  double sum = m.active ? poly_term(m.f, m.n, delta) : 0.0;
  for (int off = m.K >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
  double prod = fmax(1.0 - sum, 0.0);  // the same in all K lanes of a setting; 1 in inactive settings
  for (int off = m.TS >> 1; off >= m.K; off >>= 1) prod *= __shfl_xor(prod, off, 64);
  return prod;
}

// unit u of `units` (trial-major): lane -> entry; counts[B][R K]
__device__ inline PolyTeam poly_team_load(const int64_t* __restrict__ counts, const double* __restrict__ shots,
                                          const double* __restrict__ truth, long long trial, bool valid, int RK, int K,
                                          int kshift, int TS) {
  PolyTeam m;
  const int e = (threadIdx.x & 63) & (TS - 1);
  m.K = K;
  m.TS = TS;
  m.active = valid && e < RK;
  m.f = m.n = m.t = 0.0;
  if (m.active) {
    m.n = shots[e >> kshift];
    m.f = poly_freq(counts[trial * RK + e], m.n);
    if (truth) m.t = truth[e];
  }
  return m;
}

__global__ __launch_bounds__(256) void k_polytope_confidence_wave(const int64_t* __restrict__ counts, long long B, int R,
                                                                  int K, int kshift, int TS,
                                                                  const double* __restrict__ shots,
                                                                  const double* __restrict__ deltas, int Q,
                                                                  double* __restrict__ conf) {
  const int lane = threadIdx.x & 63, per_wave = 64 / TS;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long u = wave * per_wave + lane / TS, units = B * Q;
  const bool valid = u < units;
  const PolyTeam m = poly_team_load(counts, shots, nullptr, valid ? u / Q : 0, valid, R * K, K, kshift, TS);
  const double c = poly_team_conf(m, valid ? deltas[u] : 1.0);
  if (valid && (lane & (TS - 1)) == 0) conf[u] = c;
}

__global__ __launch_bounds__(256) void k_polytope_coverage_wave(const int64_t* __restrict__ counts, long long B, int R,
                                                                int K, int kshift, int TS,
                                                                const double* __restrict__ shots,
                                                                const double* __restrict__ levels, int L,
                                                                const double* __restrict__ truth, int clip_b,
                                                                double* __restrict__ deltas, uint8_t* __restrict__ hits) {
  const int lane = threadIdx.x & 63, per_wave = 64 / TS;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long u = wave * per_wave + lane / TS, units = B * L;
  const bool valid = u < units;
  const PolyTeam m = poly_team_load(counts, shots, truth, valid ? u / L : 0, valid, R * K, K, kshift, TS);
  const double level = valid ? levels[u % L] : 0.0;
  double left = 1e-10, right = 1.0, delta = 0.5;
  for (int it = 0; it < kPolyCap; ++it) {
    const bool go = right - left > 1e-10;
    if (!__any(go)) break;  // uniform over the wavefront: the exchanges below are made by all 64 lanes
    const double mid = (left + right) / 2;
    const double c = poly_team_conf(m, mid);
    if (go) {
      delta = mid;
      if (c < level + 1e-10) left = mid;
      else right = mid;
    }
  }
  double margin = INFINITY;
  if (truth) {
    if (m.active) margin = poly_bound(m.f, delta, clip_b) - m.t;
    for (int off = TS >> 1; off > 0; off >>= 1) margin = fmin(margin, __shfl_xor(margin, off, 64));
  }
  if (valid && (lane & (TS - 1)) == 0) {
    if (deltas) deltas[u] = delta;
    if (hits) hits[u] = truth ? (margin > -kPolyEps) : 0;
  }
}

// ---- workgroup per trial ----------------------------------------------------------------------------------------------
// Product (MIN: minimum) over the workgroup; every thread gets the same bits.  `red`: NT / 64 doubles of LDS.
template <int NT, bool MIN>
__device__ inline double poly_reduce(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = MIN ? fmin(v, o) : v * o;
  }
  if constexpr (NT > 64) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    v = red[0];
    for (int i = 1; i < NT / 64; ++i) v = MIN ? fmin(v, red[i]) : v * red[i];
  }
  return v;
}

// `fl`: the trial's frequencies in LDS (POLY_LDS) or null; `c`: the trial's counts
template <int NT, int MODE>
__device__ inline double poly_wg_conf(const PolyShape& sh, const double* fl, const int64_t* __restrict__ c,
                                      const double* __restrict__ shots, double delta, double* red) {
  const int g = threadIdx.x & (sh.G - 1), slot = threadIdx.x >> sh.gshift, slots = NT >> sh.gshift;
  double prod = 1.0;
  for (int r0 = 0; r0 < sh.R; r0 += slots) {  // the same trip count in every thread
    const int r = r0 + slot;
    double sum = 0.0;
    if (r < sh.R) {
      const double n = shots[r];
      for (int k = g; k < sh.K; k += sh.G) {
        const int i = r * sh.K + k;
        sum += poly_term(MODE == POLY_LDS ? fl[i] : poly_freq(c[i], n), n, delta);
      }
    }
    for (int off = sh.G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (r < sh.R && g == 0) prod *= fmax(1.0 - sum, 0.0);
  }
  return poly_reduce<NT, false>(prod, red);
}

template <int NT, int MODE>
__device__ inline void poly_wg_stage(const PolyShape& sh, double* fl, const int64_t* __restrict__ c,
                                     const double* __restrict__ shots) {
  if constexpr (MODE == POLY_LDS) {
    const int g = threadIdx.x & (sh.G - 1), slot = threadIdx.x >> sh.gshift, slots = NT >> sh.gshift;
    __syncthreads();  // the previous trial's readers are done
    for (int r = slot; r < sh.R; r += slots) {
      const double n = shots[r];
      for (int k = g; k < sh.K; k += sh.G) fl[r * sh.K + k] = poly_freq(c[r * sh.K + k], n);
    }
    __syncthreads();
  }
}

template <int NT, int MODE>
__global__ __launch_bounds__(NT) void k_polytope_confidence(const int64_t* __restrict__ counts, long long B, PolyShape sh,
                                                            const double* __restrict__ shots,
                                                            const double* __restrict__ deltas, int Q,
                                                            double* __restrict__ conf) {
  extern __shared__ double poly_lds[];
  double* red = poly_lds;  // 16 doubles
  double* fl = poly_lds + 16;
  const long long RK = (long long)sh.R * sh.K;
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* c = counts + b * RK;
    poly_wg_stage<NT, MODE>(sh, fl, c, shots);
    for (int q = 0; q < Q; ++q) {
      const double v = poly_wg_conf<NT, MODE>(sh, fl, c, shots, deltas[b * Q + q], red);
      if (threadIdx.x == 0) conf[b * Q + q] = v;
    }
  }
}

template <int NT, int MODE>
__global__ __launch_bounds__(NT) void k_polytope_coverage(const int64_t* __restrict__ counts, long long B, PolyShape sh,
                                                          const double* __restrict__ shots,
                                                          const double* __restrict__ levels, int L,
                                                          const double* __restrict__ truth, int clip_b,
                                                          double* __restrict__ deltas, uint8_t* __restrict__ hits) {
  extern __shared__ double poly_lds[];
  double* red = poly_lds;
  double* fl = poly_lds + 16;
  const long long RK = (long long)sh.R * sh.K;
  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    const int64_t* c = counts + b * RK;
    poly_wg_stage<NT, MODE>(sh, fl, c, shots);
    for (int l = 0; l < L; ++l) {
      const double level = levels[l];
      double left = 1e-10, right = 1.0, delta = 0.5;
      for (int it = 0; it < kPolyCap && right - left > 1e-10; ++it) {  // uniform: every thread holds the same bracket
        delta = (left + right) / 2;
        if (poly_wg_conf<NT, MODE>(sh, fl, c, shots, delta, red) < level + 1e-10) left = delta;
        else right = delta;
      }
      double margin = INFINITY;
      if (truth) {
        for (int i = threadIdx.x; i < RK; i += NT) {
          const double f = MODE == POLY_LDS ? fl[i] : poly_freq(c[i], shots[i / sh.K]);
          margin = fmin(margin, poly_bound(f, delta, clip_b) - truth[i]);
        }
        margin = poly_reduce<NT, true>(margin, red);
      }
      if (threadIdx.x == 0) {
        if (deltas) deltas[b * L + l] = delta;
        if (hits) hits[b * L + l] = truth ? (margin > -kPolyEps) : 0;
      }
    }
  }
}

// covered[l] += the number of trials whose hits[b][l] is set: one workgroup per level, partials in a fixed order
__global__ __launch_bounds__(256) void k_polytope_count(const uint8_t* __restrict__ hits, long long B, int L,
                                                        long long* __restrict__ covered) {
  __shared__ long long part[4];
  const int l = blockIdx.x;
  long long n = 0;
  for (long long b = threadIdx.x; b < B; b += 256) n += hits[b * L + l];
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) covered[l] += (part[0] + part[1]) + (part[2] + part[3]);
}

}  // namespace qt
