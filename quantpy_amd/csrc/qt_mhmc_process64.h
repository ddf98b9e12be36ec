// The chain of the coverage study for three-qubit channels (metrics.get_CL_list_channel_mhmc_large): the launch family of
// qt_mhmc_process at n = 3 (qt_process64.h) on numbers the kernels draw themselves, with the kept states measured where
// they lie -- what k_mhmc_process_hits (qt_process.h) is at n <= 2.  Per step of a slice of chains:
//   k_mhmc64_propose_draw   trial = x + step * delta, delta drawn (replaces k_mhmc64_propose and the deltas table)
//   k_cptp_project64        as it is
//   k_fwd64_nll             as it is
//   k_mhmc64_decide_hits    the uniform drawn, the accept rule, the counters, and on a kept step the Hilbert-Schmidt
//                           distance and the hit, or Re(X) parked for k_metric_dist_dim64 (replaces k_mhmc64_decide and
//                           the uniforms, chain and accepted tables)
//   k_mhmc64_tally          metric entry, kept steps: the threshold test on the distances k_metric_dist_dim64 left
// The proposal's element, the NLL from its partial sums and the accept rule are mhmc64_proposal, mhmc64_nll and
// mhmc64_accept, the device functions of the kernels they replace: on the numbers of qt_mhmc_draws_dim(dim = 4096) the
// unfused chain accepts exactly the same steps.
//
// Numbers: global step j of global chain g reads qt_sampler::mhmc_draw(seed, g, j, 4096, l) -- l < 4096 the increment of
// column-stacked entry l (element (row, col) of the row-major matrix: l = col * 64 + row, k_mhmc64_propose's index),
// l = 4096 the step's uniform, Philox block q = 2048.
//
// Geometry: one workgroup of 256 threads per chain, 16 elements per thread, element k = thread + 256 u -- a wavefront
// moves one 1 KB row of the matrix per access, 16 bytes per lane.  A wavefront's row is one value, so the parity of l,
// which picks the sine or the cosine of a Box-Muller pair, is wavefront-uniform.  The two increments of a pair, l = 2q and
// 2q + 1, belong to rows 2r and 2r + 1 of one column, that is to two wavefronts: each runs the pair's Philox block, log
// and sqrt and keeps one of the two, so the draw's arithmetic is done twice per pair (a thread that produced both would
// store to two rows, 1 KB apart; the kernel's share of a step is in profiles/process_mhmc_large_coverage_timing.txt).
// Both kernels move 64 KB per array and
// chain and are bound by memory and by the draw's arithmetic; they hold no LDS beyond the four partial sums of the
// distance.  mhmc_draw runs behind a call (mhmc_draw_call, qt_mhmc_state_large.h: the ~40 double constants of its log,
// sin and cos stay out of the caller's registers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_mhmc_state_large.h"  // mhmc_draw_call
#include "qt_process64.h"
#include "qt_sampler.h"

namespace qt {

struct Mhmc64 {
  static constexpr int DC = Pgdb64::DC, NE = Pgdb64::NE, NT = 256;
  static constexpr int kDrawLen = NE;  // the vector length of the chain's numbers: 4096 increments, then the uniform
  static_assert(NE == DC * DC && NE % NT == 0 && NT % 64 == 0 && DC == 64, "a wavefront takes one row of the matrix");
};

// What a step is to the study (the same for every chain of the launch)
struct Mhmc64Step {
  uint32_t j;     // the global step: burn-in first, then the sampling steps
  int post_burn;  // an accepted step counts
  int keep;       // the state after this step is a sample ...
  uint32_t kept;  // ... sample number `kept` of its chain
};

// trial[c] = x[c] + step * delta, delta the increments of global step j of global chain first_chain + c
__global__ void __launch_bounds__(Mhmc64::NT) k_mhmc64_propose_draw(int C, uint64_t seed, uint64_t first_chain, uint32_t j,
                                                                    double step, const double* __restrict__ x,
                                                                    double* __restrict__ trial) {
  const int c = blockIdx.x;
  if (c >= C) return;
  const cd* cur = reinterpret_cast<const cd*>(x) + (size_t)c * Mhmc64::NE;
  cd* out = reinterpret_cast<cd*>(trial) + (size_t)c * Mhmc64::NE;
  const uint64_t gc = first_chain + (uint64_t)c;
  for (int k = threadIdx.x; k < Mhmc64::NE; k += Mhmc64::NT) {
    const int row = k >> 6, col = k & 63;
    out[k] = mhmc64_proposal(cur[k], step, mhmc_draw_call(seed, gc, j, Mhmc64::kDrawLen, col * Mhmc64::DC + row));
  }
}

// The accept test of global step s.j on the tiles' partial sums, the uniform drawn; the counters accumulate in place
// (hits[] and accepted[] are zero before the first step; the launches of a stream run in order).  On a kept step:
//   parked == nullptr  hs_dst(Re(X), centres[c]) as k_hs_dist forms it -- Delta = Re(X) - centre, sum_ij Delta_ij Delta_ji
//                      by hs_term, sqrt(|sum|) / sqrt(2), 0 below 1e-15 -- the transposed element read back from the array
//                      the state was taken from (in cache: this workgroup has just read it), the order of the 4096-term
//                      sum this layout's; the hit (strict: a NaN never counts) and dist[c][s.kept]
//   parked != nullptr  Re(X) with zero imaginary parts into parked[c], for the metric kernel and k_mhmc64_tally
// The accepted state is read from `proposal` and written to `x` and the rejected one only read from `x`: no element is
// read and written by different threads.
__global__ void __launch_bounds__(Mhmc64::NT) k_mhmc64_decide_hits(int C, int nt, Mhmc64Step s, uint64_t seed,
                                                                   uint64_t first_chain, const double* __restrict__ fpart,
                                                                   const double* __restrict__ proposal, double* __restrict__ x,
                                                                   double* __restrict__ fcur,
                                                                   const double* __restrict__ centres,
                                                                   const double* __restrict__ thresholds, uint32_t n_points,
                                                                   int64_t* __restrict__ hits, int64_t* __restrict__ accepted,
                                                                   double* __restrict__ dist, double* __restrict__ parked) {
  __shared__ double red[2 * Mhmc64::NT / 64];
  const int c = blockIdx.x;
  if (c >= C) return;
  constexpr int NE = Mhmc64::NE, DC = Mhmc64::DC;
  const double fn = mhmc64_nll(fpart, c, nt);
  const double f = fcur[c];
  const double u = qt_sampler::mhmc_draw(seed, first_chain + (uint64_t)c, s.j, Mhmc64::kDrawLen, Mhmc64::kDrawLen);
  const bool acc = mhmc64_accept(u, f, fn);  // (the same bits in every thread: the branch is uniform over the workgroup)
  cd* cur = reinterpret_cast<cd*>(x) + (size_t)c * NE;
  const cd* prop = reinterpret_cast<const cd*>(proposal) + (size_t)c * NE;
  const cd* src = acc ? prop : cur;  // the state after this step
  const bool measure = s.keep && !parked;
  const cd* centre = reinterpret_cast<const cd*>(centres) + (size_t)c * NE;
  cd* park = parked ? reinterpret_cast<cd*>(parked) + (size_t)c * NE : nullptr;
  double sr = 0.0, si = 0.0;
  for (int k = threadIdx.x; k < NE; k += Mhmc64::NT) {
    const cd v = src[k];
    if (acc) cur[k] = v;
    if (measure) {
      const int kt = (k & 63) * DC + (k >> 6);
      const cd ck = centre[k], ct = centre[kt];
      const cd dl{v.re - ck.re, 0.0 - ck.im};
      const cd dt{src[kt].re - ct.re, 0.0 - ct.im};
      const cd t = hs_term(dl, dt);
      sr += t.re;
      si += t.im;
    } else if (s.keep) {
      park[k] = cd{v.re, 0.0};
    }
  }
  if (measure) {  // (launch-uniform)
    sr = gsum<64>(sr);
    si = gsum<64>(si);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[2 * w] = sr, red[2 * w + 1] = si;
  }
  __syncthreads();  // (every thread has read fcur[c]; the wavefronts' sums are in red[])
  if (threadIdx.x == 0) {
    if (acc) fcur[c] = fn;
    if (s.post_burn) accepted[c] += acc ? 1 : 0;
    if (measure) {
      const double tr = (red[0] + red[2]) + (red[4] + red[6]), ti = (red[1] + red[3]) + (red[5] + red[7]);
      double v = sqrt(hypot(tr, ti)) / sqrt(2.0);
      v = v < 1e-15 ? 0.0 : v;
      hits[c] += thresholds[c] > v ? 1 : 0;
      if (dist) dist[(size_t)c * n_points + s.kept] = v;
    }
  }
}

// Metric entry, after k_metric_dist_dim64 on the parked states of a kept step: hits[c] += thresholds[c] > value[c]
// (strict: a NaN never counts) and dist[c][kept] (nullable) = value[c]
__global__ void __launch_bounds__(256) k_mhmc64_tally(int C, const double* __restrict__ value,
                                                      const double* __restrict__ thresholds, uint32_t n_points, uint32_t kept,
                                                      int64_t* __restrict__ hits, double* __restrict__ dist) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double v = value[c];
  hits[c] += thresholds[c] > v ? 1 : 0;
  if (dist) dist[(size_t)c * n_points + kept] = v;
}

}  // namespace qt
