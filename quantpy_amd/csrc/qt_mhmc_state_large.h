// The chain of the coverage study at n = 4, 5 (metrics.get_CL_list_state_mhmc): k_mhmc_state_large (qt_large.h) on
// numbers the threads draw themselves, with the kept states measured where they are held -- qt_mhmc_state.h one level up.
//
// One workgroup of D = 4^n threads per chain, thread t owns x[t].  Global step j of global chain first_chain + b:
//   thread t draws its increment mhmc_draw(seed, chain, j, D, t); every thread draws the step's uniform
//   mhmc_draw(seed, chain, j, D, D) -- the same bits in all of them, as f and fn are (Large::bsum) -- so the accept branch
//   is uniform over the workgroup.  No barrier sits under a condition that is not uniform over the launch or the workgroup.
// The step is k_mhmc_state_large's, operand for operand: fma(step, delta, x), sqrt(bsum(xp^2)), the division,
// nll_value_inl, exp(f - fn), u <= alpha; the unfused chain on the numbers of qt_mhmc_draws_dim accepts the same steps.
// Steps j < burn_steps are burn-in; of the n_points * thinning steps behind them post-burn step s is kept when
// s % thinning == 0 (mhmc_state_hits_body).  On a kept step the thread forms its element of L L^dagger by
// Large::build_llh, as k_chol_unparam_large does, and the workgroup the distance to centres[b]:
//   hits[b] = #{ kept : thresholds[b] > distance }  (strict: a NaN never counts),  accepted[b] = accepted post-burn steps,
//   dist[b][k] (nullable) = the distance of kept state k.
// Thread 0 counts in registers and stores once.
//
// LDS: the chain's own (Large<NQ>::lds_bytes, large_plan in qtomo.hip) and nothing more.  In the order of the allocation:
//   L | vec | lam | red[32] | line-search slots | tabT, tabP | X | Y | (n = 5: the 32-bit count cache, PovmView::extra)
// A distance works in X and Y, the scratch of the evaluation, dead between two evaluations: the Hilbert-Schmidt distance
// sends Delta^T through Aimg() = Y; the MetricDim<2^n> functions take Aimg() / Vimg() = Y / X as their two images (the same
// pitch d + 1 and at least the same size) and the first 16 of the 32 slots of red[] for their sums.  What a chain keeps from
// step to step lies outside both images: the POVM tables tabT / tabP in front of X, the count cache behind Y, and x, f and
// the counters in registers.  build_llh's L and vec are rewritten by every evaluation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_large.h"
#include "qt_metric_dim.h"
#include "qt_sampler.h"

namespace qt {

// mhmc_draw as a call.  Inlined into the step loop, the ~40 double constants of its log, sin and cos are hoisted out of
// the loop into registers of their own, which at n = 5 (1024 threads: 128 VGPRs) the evaluation has not got to spare: the
// kernels spilled 20-23 registers, reloaded inside every step.  Behind a call the constants live in the callee alone.
__device__ __attribute__((noinline)) inline double mhmc_draw_call(uint64_t seed, uint64_t chain, uint32_t step, int D, int l) {
  return qt_sampler::mhmc_draw(seed, chain, step, D, l);
}

// `distance(c, m, centre)`: the workgroup's distance of the kept state (this thread's element m) to its centre, the same
// bits in every thread.  Called by all threads, on a launch-uniform condition.
template <int NQ, class Dist>
__device__ __forceinline__ void mhmc_state_large_hits_body(PovmView pv, const int64_t* __restrict__ counts, int C,
                                                           const double* __restrict__ centres,
                                                           const double* __restrict__ x_init,
                                                           const double* __restrict__ thresholds, uint64_t seed,
                                                           uint64_t first_chain, uint32_t burn_steps, uint32_t n_points,
                                                           uint32_t thinning, double step, int64_t* __restrict__ hits,
                                                           int64_t* __restrict__ accepted, double* __restrict__ dist,
                                                           Dist distance) {
  using S = Large<NQ>;
  constexpr int D = S::D;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x;
  if (b >= C) return;
  typename S::Ctx c;
  S::make_ctx(c, smem, pv, counts + (size_t)b * pv.M);
  double x = x_init[(size_t)b * D + c.t];
  double f = S::nll_value_inl(c, x);
  const uint64_t gc = first_chain + (uint64_t)b;
  const double* centre = centres + (size_t)b * 2 * D;
  const double thr = thresholds[b];
  int64_t n_hit = 0, n_acc = 0;
  uint32_t kept = 0, to_keep = 0;  // to_keep: steps until the next kept one
  const uint32_t total = burn_steps + n_points * thinning;  // (< 2^32 - 1: checked by the entry)
  for (uint32_t j = 0; j < total; ++j) {
    // the LDS base and the per-thread indices laundered through an empty asm every step, as in k_mhmc_state_large: else
    // hipcc hoists the loop-invariant LDS addresses of the evaluation out of the loop and spills them
    typename S::Ctx ci = c;
    {
      int off = 0, v0 = 0;
      asm volatile("" : "+s"(off));
      ci.sm = c.sm + off;
      asm volatile("" : "+v"(v0));
      ci.t = c.t + v0, ci.i = c.i + v0, ci.j = c.j + v0, ci.e = c.e + v0;
      ci.xm = c.xm + v0, ci.zm = c.zm + v0, ci.ny = c.ny + v0, ci.pi = c.pi + v0, ci.pj = c.pj + v0;
    }
    const double xp = fma(step, mhmc_draw_call(seed, gc, j, D, c.t), x);
    const double nrm = sqrt(S::bsum(ci, xp * xp));
    const double xn = xp / nrm;
    const double fn = S::nll_value_inl(ci, xn);
    const double alpha = exp(f - fn);
    // (drawn behind the evaluation: nothing of it is live across that)
    const bool acc = qt_sampler::mhmc_draw(seed, gc, j, D, D) <= alpha;  // false for a NaN alpha, like the reference's
    if (acc) {
      x = xn;
      f = fn;
    }
    if (j >= burn_steps) {  // (launch-uniform, as is the kept-step test)
      n_acc += acc;
      if (to_keep == 0) {
        double tr;
        const cd m = S::build_llh(ci, x, tr);
        const double v = distance(ci, m, centre);
        n_hit += thr > v;
        if (dist && c.t == 0) dist[(size_t)b * n_points + kept] = v;
        ++kept;
        to_keep = thinning;
      }
      --to_keep;
    }
  }
  if (c.t == 0) {
    hits[b] = n_hit;
    accepted[b] = n_acc;
  }
}

// hs_dst(L L^dagger, centre) as k_hs_dist defines it (qt_hs_dist_dim): sum_ij Delta_ij Delta_ji by hs_term, the transposed
// element through the Y image, sqrt(|sum|) / sqrt(2), 0 below 1e-15.  The order of the d^2-term sum is this layout's.
template <int NQ>
__device__ __forceinline__ double mhmc_large_hs_to_centre(const typename Large<NQ>::Ctx& c, cd m,
                                                          const double* __restrict__ centre) {
  using S = Large<NQ>;
  const double2 cc = *reinterpret_cast<const double2*>(centre + 2 * c.t);
  const cd dl{m.re - cc.x, m.im - cc.y};
  cd* A = c.Aimg();  // (its last readers, the stages of the evaluation, lie behind the barriers of build_llh)
  A[c.e] = dl;
  __syncthreads();
  const cd dt = A[c.j * S::LD + c.i];
  const cd tm = hs_term(dl, dt);
  const double sr = S::bsum(c, tm.re);  // (barriers inside: every read of A is done before the next evaluation writes)
  const double si = S::bsum(c, tm.im);
  const double v = sqrt(hypot(sr, si)) / sqrt(2.0);
  return v < 1e-15 ? 0.0 : v;
}

template <int NQ>
__global__ void __launch_bounds__(Large<NQ>::NT) k_mhmc_state_large_hits(
    PovmView pv, const int64_t* __restrict__ counts, int C, const double* __restrict__ centres,
    const double* __restrict__ x_init, const double* __restrict__ thresholds, uint64_t seed, uint64_t first_chain,
    uint32_t burn_steps, uint32_t n_points, uint32_t thinning, double step, int64_t* __restrict__ hits,
    int64_t* __restrict__ accepted, double* __restrict__ dist) {
  mhmc_state_large_hits_body<NQ>(pv, counts, C, centres, x_init, thresholds, seed, first_chain, burn_steps, n_points, thinning,
                                 step, hits, accepted, dist,
                                 [](const typename Large<NQ>::Ctx& c, cd m, const double* __restrict__ centre) {
                                   return mhmc_large_hs_to_centre<NQ>(c, m, centre);
                                 });
}

// The same chain with the kept states measured in trace distance or infidelity (qt_mhmc_state_large_metric_hits): the
// value k_metric_dist_dim returns for L L^dagger and centres[b], by the same device functions on the chain's X / Y images.
// METRIC = kMetricInfidelity: `centres` holds the roots k_psd_sqrt_dim made of them.
template <int NQ, int METRIC>
__global__ void __launch_bounds__(Large<NQ>::NT) k_mhmc_state_large_metric_hits(
    PovmView pv, const int64_t* __restrict__ counts, int C, const double* __restrict__ centres,
    const double* __restrict__ x_init, const double* __restrict__ thresholds, uint64_t seed, uint64_t first_chain,
    uint32_t burn_steps, uint32_t n_points, uint32_t thinning, double step, int64_t* __restrict__ hits,
    int64_t* __restrict__ accepted, double* __restrict__ dist) {
  using S = Large<NQ>;
  using W = MetricDim<S::d>;
  static_assert(W::LD == S::LD && W::MAT == S::MAT && W::NT == S::NT, "the metric's images are Large's Aimg() / Vimg()");
  const double jtol2 = pv.jtol2;
  mhmc_state_large_hits_body<NQ>(pv, counts, C, centres, x_init, thresholds, seed, first_chain, burn_steps, n_points, thinning,
                                 step, hits, accepted, dist,
                                 [jtol2](const typename S::Ctx& c, cd m, const double* __restrict__ centre) {
                                   typename W::CtxAt mc;
                                   W::make_ctx(mc, c.Aimg(), c.Vimg(), c.red(), jtol2);
                                   mc.t = c.t, mc.i = c.i, mc.j = c.j, mc.e = c.e;  // (the step's laundered indices)
                                   const cd q{centre[2 * c.t], centre[2 * c.t + 1]};
                                   return METRIC == kMetricTrace ? W::trace_dist(mc, m, q) : W::infidelity(mc, m, q);
                                 });
}

}  // namespace qt
