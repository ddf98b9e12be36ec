// Metropolis-Hastings chains on the Cholesky parameters of a state, n <= 3, over Small<NQ> (qt_small.h): the chain on
// numbers drawn by the host (k_mhmc_state) and the chain of the coverage study, which draws its own (k_mhmc_state_hits,
// qt_sampler::mhmc_draw).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_sampler.h"
#include "qt_small.h"

namespace qt {

// Metropolis-Hastings chain on the Cholesky parameters (reference mhmc.py:80-119 with
// `normalized_update`, interval.py:735-750): one chain per lane group.  Step t, from the increment delta_t of this lane's
// parameter and the uniform u_t of the chain (mhmc_step, the one body of both kernels below):
//   x' = (x + step * delta_t) / ||x + step * delta_t||,  alpha = exp(nll(x) - nll(x')),  accept iff u_t <= alpha.
// x, f: the state and its NLL, replaced on acceptance.  Executed by every lane of the wavefront.
template <int NQ, class C>
__device__ __forceinline__ bool mhmc_step(const C& c, double step, double delta, double u, double& x, double& f) {
  using S = Small<NQ>;
  const double xp = fma(step, delta, x);
  const double nrm = sqrt(gsum<S::G>(xp * xp));
  const double xn = xp / nrm;
  double fn, unused;
  S::nll_grad(c, xn, fn, unused, nullptr, false);
  const double alpha = exp(f - fn);
  const bool acc = u <= alpha;  // false for a NaN alpha, like the reference's comparison
  if (acc) {
    x = xn;
    f = fn;
  }
  return acc;
}

// The increments and the uniforms drawn on the host in the reference's order:
// chain[c][t][:] = the state AFTER step t, accepted[c][t] = 0 / 1.
template <int NQ>
__global__ void __launch_bounds__(256) k_mhmc_state(PovmView pv, const int64_t* __restrict__ counts, int C,
                                                    const double* __restrict__ x_init, const double* __restrict__ deltas,
                                                    const double* __restrict__ uniforms, int T_steps, double step,
                                                    double* __restrict__ chain, int32_t* __restrict__ accepted) {
  using S = Small<NQ>;
  constexpr int D = S::D;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  S::make_ctx(c, smem, pv);
  bool live;
  const int b = S::trial_index(C, &live);
  const int bb = live ? b : C - 1;
  S::load_freq(c, counts + (size_t)bb * pv.M);
  double x = x_init[(size_t)bb * D + c.l];
  double f, unused;
  S::nll_grad(c, x, f, unused, nullptr, false);
  const double* dl = deltas + (size_t)bb * T_steps * D + c.l;
  const double* un = uniforms + (size_t)bb * T_steps;
  for (int t = 0; t < T_steps; ++t) {
    const bool acc = mhmc_step<NQ>(c, step, dl[(size_t)t * D], un[t], x, f);
    if (live) {
      chain[((size_t)b * T_steps + t) * D + c.l] = x;
      if (c.l == 0) accepted[(size_t)b * T_steps + t] = acc ? 1 : 0;
    }
  }
}

// The chain of the coverage study (metrics.get_CL_list_state_mhmc): the same steps on numbers the lanes draw themselves
// (qt_sampler::mhmc_draw, global chain first_chain + b, global step = burn-in steps first, then the n_points * thinning
// sampling steps), and of the chain only three numbers per trial leave the registers.  Post-burn step s is kept when
// s % thinning == 0 (mhmc.py:80-84); on a kept step the lane forms its element of L L^dagger as k_chol_unparam does and
// the group its distance to centres[b] (k_mhmc_state_hits: Hilbert-Schmidt, hs_to_centre):
//   hits[b] = #{ kept : thresholds[b] > distance }  (strict: a NaN never counts),  accepted[b] = accepted post-burn steps,
//   dist[b][k] (nullable) = the distance of kept state k.
// Lane 0 of a live group counts in registers and stores once; every lane runs the distance and the reductions.
// `distance(c, m, centre)`: the group's distance of the kept state to its centre, the same bits in every lane of the group.
template <int NQ, class Dist>
__device__ __forceinline__ void mhmc_state_hits_body(PovmView pv, const int64_t* __restrict__ counts, int C,
                                                     const double* __restrict__ centres, const double* __restrict__ x_init,
                                                     const double* __restrict__ thresholds, uint64_t seed,
                                                     uint64_t first_chain, uint32_t burn_steps, uint32_t n_points,
                                                     uint32_t thinning, double step, int64_t* __restrict__ hits,
                                                     int64_t* __restrict__ accepted, double* __restrict__ dist,
                                                     Dist distance) {
  using S = Small<NQ>;
  constexpr int D = S::D;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::Ctx c;
  S::make_ctx(c, smem, pv);
  bool live;
  const int b = S::trial_index(C, &live);
  const int bb = live ? b : C - 1;
  S::load_freq(c, counts + (size_t)bb * pv.M);
  double x = x_init[(size_t)bb * D + c.l];
  double f, unused;
  S::nll_grad(c, x, f, unused, nullptr, false);
  const uint64_t gc = first_chain + (uint64_t)bb;
  const double* centre = centres + (size_t)bb * 2 * D;
  const double thr = thresholds[bb];
  const bool writer = live && c.l == 0;
  uint32_t j = 0;
  for (; j < burn_steps; ++j)
    mhmc_step<NQ>(c, step, qt_sampler::mhmc_draw(seed, gc, j, D, c.l), qt_sampler::mhmc_draw(seed, gc, j, D, D), x, f);
  int64_t n_hit = 0, n_acc = 0;
  uint32_t kept = 0, to_keep = 0;  // to_keep: steps until the next kept one
  const uint32_t total = n_points * thinning;  // (< 2^32 - 1 with the burn-in: checked by the entry)
  for (uint32_t s = 0; s < total; ++s, ++j) {
    n_acc += mhmc_step<NQ>(c, step, qt_sampler::mhmc_draw(seed, gc, j, D, c.l), qt_sampler::mhmc_draw(seed, gc, j, D, D), x, f);
    if (to_keep == 0) {  // (launch-uniform)
      double tr;
      const cd m = S::build_llh(c, x, tr);
      const double v = distance(c, m, centre);
      n_hit += thr > v;
      if (dist && writer) dist[(size_t)b * n_points + kept] = v;
      ++kept;
      to_keep = thinning;
    }
    --to_keep;
  }
  if (writer) {
    hits[b] = n_hit;
    accepted[b] = n_acc;
  }
}

template <int NQ>
__global__ void __launch_bounds__(256) k_mhmc_state_hits(PovmView pv, const int64_t* __restrict__ counts, int C,
                                                         const double* __restrict__ centres, const double* __restrict__ x_init,
                                                         const double* __restrict__ thresholds, uint64_t seed,
                                                         uint64_t first_chain, uint32_t burn_steps, uint32_t n_points,
                                                         uint32_t thinning, double step, int64_t* __restrict__ hits,
                                                         int64_t* __restrict__ accepted, double* __restrict__ dist) {
  using S = Small<NQ>;
  mhmc_state_hits_body<NQ>(pv, counts, C, centres, x_init, thresholds, seed, first_chain, burn_steps, n_points, thinning, step,
                           hits, accepted, dist, [](const typename S::Ctx& c, cd m, const double* __restrict__ centre) {
                             return S::hs_to_centre(c, m, centre);
                           });
}

// The same chain with the kept states measured in trace distance or infidelity (qt_mhmc_state_metric_hits): the value
// k_metric_dist returns for L L^dagger and centres[b], by the same device functions (Small::trace_dist, Small::infidelity
// on jacobi_sweeps<OWN>: at n = 1 sixteen chains share a wavefront, at n = 2 four, and a chain's bits do not depend on
// how many sweeps its neighbours take).  METRIC = kMetricInfidelity: `centres` holds the roots k_psd_sqrt made of them.
// The sweeps' two matrix images are the chain context's own A() and V(): scratch of nll_grad and build_llh, whose last
// reads lie behind a wave_sync by the time the kept state's element is returned; the frequencies, the one thing a chain
// keeps in LDS from step to step, lie behind them (V() is on rbuf or has a block of its own, Small::v_offset).
template <int NQ, int METRIC>
__global__ void __launch_bounds__(256) k_mhmc_state_metric_hits(PovmView pv, const int64_t* __restrict__ counts, int C,
                                                                const double* __restrict__ centres,
                                                                const double* __restrict__ x_init,
                                                                const double* __restrict__ thresholds, uint64_t seed,
                                                                uint64_t first_chain, uint32_t burn_steps, uint32_t n_points,
                                                                uint32_t thinning, double step, int64_t* __restrict__ hits,
                                                                int64_t* __restrict__ accepted, double* __restrict__ dist) {
  using S = Small<NQ>;
  mhmc_state_hits_body<NQ>(pv, counts, C, centres, x_init, thresholds, seed, first_chain, burn_steps, n_points, thinning, step,
                           hits, accepted, dist, [](const typename S::Ctx& c, cd m, const double* __restrict__ centre) {
                             const cd q{centre[2 * c.l], centre[2 * c.l + 1]};
                             return METRIC == kMetricTrace ? S::trace_dist(c, m, q) : S::infidelity(c, m, q);
                           });
}

}  // namespace qt
