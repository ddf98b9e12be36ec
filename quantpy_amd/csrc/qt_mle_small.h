// The MLE drivers for n <= 3 over Small<NQ> (qt_small.h): the split pair k_mle_start / k_mle_bfgs, the BFGS loop with
// its two forms of the inverse Hessian (DenseH, TwoLoop), and the one-launch kernels k_mle_fused / k_mle_fused_mixed /
// k_mle_fused_hw (twin wavefront per trial).  scipy's BFGS control flow is qt_linesearch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "qt_linesearch.h"
#include "qt_small.h"

namespace qt {

// What the start of a trial asks of its first gradient's max-norm: whether it is above gtol (the trial iterates) and
// whether it is a NaN (mle_start_status reads it for nothing else).  The specialised n = 3 kernels answer with two
// ballots -- gnorm > gtol <=> no element is a NaN and some element is above; gnorm != gnorm <=> some element is a
// NaN -- and hand mle_start_status 0 or a NaN in place of the norm: the v_max_f64 butterfly of gmax stood between the
// evaluation and the stores of every trial.  (The BFGS loop's norms are gmax: bfgs_step_exit compares them.)
template <int NQ, bool GENERIC>
constexpr bool kStartBallots = NQ == 3 && !GENERIC && kLaneLeftovers;
template <int G>
__device__ __forceinline__ double start_norm_ballots(double gk, double gtol, bool& above) {
  const bool nan = group_any<G>(gk != gk);
  above = !nan && group_any<G>(fabs(gk) > gtol);
  return nan ? __builtin_nan("") : 0.0;
}

// a10, part 1: starting point (state.py:205-212), Cholesky parametrisation and the first
// (value, gradient) evaluation.  Trials whose gradient already meets gtol -- every full-rank
// high-shot trial, where BFGS exits at iteration 0 -- are finished here; the
// rest hand x0, g0, f0 to k_mle_bfgs.  Keeping the D x D inverse Hessian out of this kernel
// keeps its register footprint small.
// Held to four wavefronts per SIMD (128 VGPRs): the saturated batches run four workgroups per CU, and one
// register more -- the EstOut pointers of round 3 made it 129 -- takes a workgroup off every CU (measured: 0.372 -> 0.416 ms
// per 65 536 trials).
template <int NQ, bool GENERIC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_mle_start(const int64_t* __restrict__ counts, const void* image, const double* Ns, int B, int M, int extra,
                                                   int max_iter, double gtol, typename MleArgs<GENERIC>::type pv0, int init, EstOut rho,
                                                   int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                                   double* __restrict__ fun_out, int32_t* __restrict__ status_out,
                                                   double* __restrict__ ws_x, double* __restrict__ ws_g,
                                                   double* __restrict__ ws_f, int32_t* __restrict__ ws_active) {
  using S = Small<NQ>;
  constexpr int D = S::D, G = S::G, d = S::d;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  typename S::template CtxOf<GENERIC>::type c;
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;
  const auto pv = mle_front(pv0, image, Ns, M, extra);
  typename S::Prefetch pf;
  S::prefetch_counts(pf, counts + (size_t)bb * pv.M, pv);
  if constexpr (!GENERIC) S::take_coefs(c, pv);
  bool shots_ok;
  if constexpr (GENERIC) {
    S::make_ctx(c, smem, pv);
    shots_ok = S::load_freq(c, counts + (size_t)bb * pv.M, &pf);
  } else {
    S::make_ctx(c, smem, pv, pf);
    shots_ok = S::load_freq(c, pf);
  }
  int ok;
  double xk;
  typename S::StartPoint sp;
  if (init == 0) {
    double bl;
    const cd lin = S::lin_invert(c, bl);
    sp.rho = S::make_feasible(c, lin, &xk, &ok, &sp.lscale);  // physical 'lin' estimate, Cholesky-parametrised
  } else {
    sp.rho = cd{c.i == c.j ? 1.0 / d : 0.0, 0.0};
    sp.lscale = 1.0;
    xk = S::cholesky_param(c, sp.rho, ok);
  }
  double fk, gk;
  cd rho_l;  // L L^dagger / Tr at x_k: what the trial returns if BFGS does not move
  [[maybe_unused]] typename S::DeferredValue dv;
  if constexpr (GENERIC) S::nll_grad(c, xk, fk, gk, &rho_l, true, &sp);
  else S::template nll_grad<true>(c, xk, fk, gk, &rho_l, true, &sp, &dv);
  double gnorm;
  bool iterate;
  if constexpr (kStartBallots<NQ, GENERIC>) {
    bool above;
    gnorm = start_norm_ballots<G>(gk, gtol, above);
    iterate = shots_ok && ok && above && (0 < max_iter);
  } else {
    gnorm = gmax<G>(fabs(gk));
    iterate = shots_ok && ok && (gnorm > gtol) && (0 < max_iter);
  }
  if constexpr (!GENERIC) fk = S::value_if_needed(c, dv, iterate || fun_out != nullptr);
  const int status = mle_start_status(shots_ok, ok, iterate, max_iter, gnorm, fk, group_any<G>(xk != xk));
  S::emit(c, rho, b, live, rho_l);
  if (live) {
    if (iterate) {  // the hand-off is written only for trials that go on to k_mle_bfgs
      ws_x[(size_t)b * D + c.l] = xk;
      ws_g[(size_t)b * D + c.l] = gk;
    }
    if (c.l == 0) {
      if (iterate) ws_f[b] = fk;
      ws_active[b] = iterate ? 1 : 0;
      store_trial(b, 0, ok ? 1 : 0, fk, status, nit_out, nfev_out, fun_out, status_out);
    }
  }
}

// a10, part 2: the BFGS iterations (scipy _minimize_bfgs) of the trials whose first gradient did not
// meet gtol.  One (value, gradient) evaluation per loop pass; the line search is the state machine of
// qt_linesearch.h, whose scalar rules (bfgs_*) this loop shares with the n = 4, 5 kernel (qt_large.h).  `mine` marks
// the groups that iterate; the others idle through the evaluations on finite dummy values.
// ONE loop for both forms of the inverse Hessian; `Dir` says how p = -H g is formed behind an accepted step:
//   double next(c, np, sk, yk, gk, rhok)  this lane's element of the next direction; (sk, yk, rhok) is pair `np`
//   kLsInLds                              the caller's LineSearch lives in LDS, shared by the lanes of the group: the
//                                         loop orders its writes before the next pass's reads
template <int NQ, class Dir, class C>
__device__ __forceinline__ void bfgs_loop(const C& c, Dir& dir, LineSearch& ls, bool mine, double xk, double gk,
                                          double fk, int b, int max_iter, double gtol, EstOut rho,
                                          int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                          double* __restrict__ fun_out, int32_t* __restrict__ status_out) {
  using S = Small<NQ>;
  constexpr int G = S::G;
  bool active = mine;
  double old_old = fk + sqrt(gsum<G>(gk * gk)) / 2.0;
  double pk = -gk, stp = 0.0;  // H0 = I
  int kiter = 0, nfev = 1, status = TRIAL_OK;
  ls.start(fk, old_old, gsum<G>(gk * pk), &stp);
  if constexpr (Dir::kLsInLds) wave_sync();
  const int eval_cap = bfgs_eval_cap(max_iter);

#ifdef QT_PHASE_TIMING  // slots 21 / 22: clocks in this loop / inside its nll_grad calls; 23 / 24: iterations, evaluations
  long long t_nll = 0;
  const long long t_loop0 = (long long)__builtin_readcyclecounter();
#endif
  while (__any(active)) {  // per wave: the waves of a workgroup do not synchronise here
    double ft, gt;
#ifdef QT_PHASE_TIMING
    const long long t_e0 = (long long)__builtin_readcyclecounter();
#endif
    S::nll_grad(c, xk + stp * pk, ft, gt);  // executed by the whole wave; finished trials idle through it
#ifdef QT_PHASE_TIMING
    t_nll += (long long)__builtin_readcyclecounter() - t_e0;
#endif
    if (active && ++nfev > eval_cap) {
      status = TRIAL_LINESEARCH;
      active = false;
    }
    if (active) {
      const double dphi = gsum<G>(gt * pk);
      double next = stp;
      const int r = ls.advance(stp, ft, dphi, &next);
      if (r == LS_EVAL) {
        stp = next;
      } else if (r == LS_FAIL) {
        status = TRIAL_LINESEARCH;
        active = false;
      } else {
        // step accepted: x += s, y = g_new - g
        const double sk = stp * pk;
        const double pnorm2 = gsum<G>(pk * pk);
        xk = xk + sk;
        const double yk = gt - gk;
        gk = gt;
        old_old = fk;
        fk = ft;
        ++kiter;
        const double gnorm = gmax<G>(fabs(gk));
        if (bfgs_step_exit(gnorm, gtol, stp, pnorm2, fk, kiter, max_iter, &status)) {
          active = false;
        } else {
          pk = dir.next(c, kiter - 1, sk, yk, gk, bfgs_rho(gsum<G>(yk * sk)));
          ls.start(fk, old_old, gsum<G>(gk * pk), &stp);
        }
      }
    }
    if constexpr (Dir::kLsInLds) wave_sync();
  }
#ifdef QT_PHASE_TIMING
  QT_STAMP_VAL(21, (long long)__builtin_readcyclecounter() - t_loop0);
  QT_STAMP_VAL(22, t_nll);
  QT_STAMP_VAL(23, (long long)kiter);
  QT_STAMP_VAL(24, (long long)nfev);
#endif
  status = bfgs_final_status(status, kiter, max_iter, gmax<G>(fabs(gk)), fk, gmax<G>(fabs(xk)));
  // ---- result: L L^dagger / Tr  (state.py:214-215)
  double tr;
  const cd m = S::build_llh(c, xk, tr);
  S::emit(c, rho, b, mine, cd{m.re / tr, m.im / tr});
  if (mine && c.l == 0) store_trial(b, kiter, nfev, fk, status, nit_out, nfev_out, fun_out, status_out);
}

// The inverse Hessian itself, one row per lane in registers (n = 1, 2: 4 / 16 doubles): the rank-two update with the
// new pair, then the product with the gradient.
template <int NQ>
struct DenseH {
  static constexpr bool kLsInLds = false;
  static constexpr int D = Small<NQ>::D, G = Small<NQ>::G;
  double H[D];
  template <class C>
  __device__ __forceinline__ explicit DenseH(const C& c) {
#pragma unroll
    for (int k = 0; k < D; ++k) H[k] = (k == c.l) ? 1.0 : 0.0;
  }
  template <class C>
  __device__ __forceinline__ double next(const C& c, int, double sk, double yk, double gk, double rhok) {
    double* vec = c.vec();
    // H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T, expanded with u = H y
    vec[c.l] = yk;
    wave_sync();
    // four partial sums: a lone wave pays ~16 ns per DEPENDENT FP64 instruction under load
    // (profiles/round1_v14_ubench_valu_f64.txt); a 64-term chain would be 1 us of latency
    double uu[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) uu[k & 3] = fma(H[k], vec[k], uu[k & 3]);
    double u = (uu[0] + uu[1]) + (uu[2] + uu[3]);
    const double yhy = gsum<G>(yk * u);
    wave_sync();
    double* ubuf = reinterpret_cast<double*>(c.A());  // 2 D doubles: u | s
    ubuf[c.l] = u;
    ubuf[D + c.l] = sk;
    wave_sync();
    const double cc = rhok * rhok * yhy + rhok;
    // (regrouped as H_lk += a_l s_k + b_l u_k with (u_k, s_k) read as one 16-byte pair: two FMAs per element
    //  instead of five operations, and measured 6 % SLOWER per iteration -- scripts/bfgs_phase_timing.py)
#pragma unroll
    for (int k = 0; k < D; ++k)
      H[k] += -rhok * (u * ubuf[D + k] + sk * ubuf[k]) + cc * sk * ubuf[D + k];
    wave_sync();
    vec[c.l] = gk;
    wave_sync();
    double hh[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < D; ++k) hh[k & 3] = fma(H[k], vec[k], hh[k & 3]);
    const double hp = (hh[0] + hh[1]) + (hh[2] + hh[3]);
    wave_sync();
    return -hp;
  }
};

// WITHOUT the inverse Hessian in registers, for batches that fill the chip (k_mle_bfgs): with H_0 = I the matrix
// scipy updates, H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T, is exactly the product form the two-loop
// recursion evaluates, so p = -H_k g is computed from the (s_i, y_i) pairs of the accepted steps (as at n = 4, 5,
// qt_large.h, under the same rules of qt_linesearch.h).  Lane l only ever touches element l of each pair: private,
// coalesced streams in a global workspace `pairs` [B][max_iter][2][D] that stay in L2; rho_i, alpha_i and -- across
// every evaluation -- the line-search state live in the trial's LDS (`pv.extra` doubles).  Registers: ~150 instead
// of 256 + 91 AGPRs, i.e. three waves per SIMD instead of one, and 2 k reductions + 4 k FMAs per iteration instead
// of two 64-term products and a 64-entry rank-two update.  Same iterates as the dense form to rounding
// (tests/test_gpu_state.py runs the reference's 70 golden trials through both).
// LP > 0 (k_mle_fused: one workgroup per CU, LDS to spare): the first LP pairs stay in the trial's LDS and only later
// ones go to the global workspace -- a lone wave would otherwise wait out an L2 round trip per block of pairs.
template <int NQ, int LP>
struct TwoLoop {
  static constexpr bool kLsInLds = true;
  static constexpr int D = Small<NQ>::D, G = Small<NQ>::G;
  double* my;      // s_i[l] at my[2 i D], y_i[l] at my[(2 i + 1) D]
  double* prho;    // [max_iter]
  double* palpha;  // [max_iter]
  double* lp;      // [LP][2][D]: s_i[l] at lp[2 i D], y_i[l] at lp[(2 i + 1) D]
  template <class C>
  __device__ __forceinline__ TwoLoop(const C& c, double* __restrict__ pairs, int b, int max_iter)
      : my(pairs + (size_t)b * max_iter * 2 * D + c.l),
        prho(c.extra() + LineSearch::SLOTS),
        palpha(prho + max_iter),
        lp(palpha + max_iter + c.l) {}
  template <class C>
  __device__ __forceinline__ double next(const C& c, int np, double sk, double yk, double gk, double rhok) {
    if (np < LP) {
      lp[(2 * np) * D] = sk;
      lp[(2 * np + 1) * D] = yk;
    } else {
      my[(size_t)(2 * np) * D] = sk;
      my[(size_t)(2 * np + 1) * D] = yk;
    }
    if (c.l == 0) prho[np] = rhok;
    wave_sync();
    double q = gk;
    for (int i = np; i >= 0; --i) {
      double si = sk, yi = yk;
      if (i != np) {
        if (i < LP) {
          si = lp[(2 * i) * D];
          yi = lp[(2 * i + 1) * D];
        } else {
          si = my[(size_t)(2 * i) * D];
          yi = my[(size_t)(2 * i + 1) * D];
        }
      }
      const double a = prho[i] * gsum<G>(si * q);
      if (c.l == 0) palpha[i] = a;
      q = fma(-a, yi, q);
    }
    wave_sync();
    for (int i = 0; i <= np; ++i) {
      double si = sk, yi = yk;
      if (i != np) {
        if (i < LP) {
          si = lp[(2 * i) * D];
          yi = lp[(2 * i + 1) * D];
        } else {
          si = my[(size_t)(2 * i) * D];
          yi = my[(size_t)(2 * i + 1) * D];
        }
      }
      const double bb = prho[i] * gsum<G>(yi * q);
      q = fma(si, palpha[i] - bb, q);
    }
    return -q;
  }
};

template <int NQ, class C>
__device__ __forceinline__ void bfgs_iterate(const C& c, bool mine, double xk, double gk,
                                             double fk, int b, int max_iter, double gtol, EstOut rho,
                                             int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                             double* __restrict__ fun_out, int32_t* __restrict__ status_out) {
  DenseH<NQ> dir(c);
  LineSearch ls;
  bfgs_loop<NQ>(c, dir, ls, mine, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out);
}

template <int NQ, int LP = 0, class C>
__device__ __forceinline__ void bfgs_iterate_2l(const C& c, bool mine, double xk, double gk,
                                                double fk, int b, int max_iter, double gtol, EstOut rho,
                                                int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                                double* __restrict__ fun_out, int32_t* __restrict__ status_out,
                                                double* __restrict__ pairs) {
  TwoLoop<NQ, LP> dir(c, pairs, b, max_iter);
  // The line-search state lives IN LDS (every lane of the group reads and writes the same words with the same values):
  // as a register-resident struct its ~35 doubles plus the temporaries of dcstep made the allocation 240 VGPRs.
  static_assert(sizeof(LineSearch) <= LineSearch::SLOTS * sizeof(double), "LDS slot of the line-search state");
  LineSearch& ls = *reinterpret_cast<LineSearch*>(c.extra());
  bfgs_loop<NQ>(c, dir, ls, mine, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out);
}

#ifndef QT_BFGS_WAVES
#define QT_BFGS_WAVES 2  // waves per SIMD the BFGS kernel is compiled for; measured at B = 65 536 (15-iteration trials): 3 waves
                         // (<= 168 VGPRs, 18 spilled) 5.29 ms, 2 waves (205 VGPRs, no scratch) 5.39 ms -- instruction-bound either way
#endif
template <int NQ, bool GENERIC>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(QT_BFGS_WAVES))) k_mle_bfgs(const int64_t* __restrict__ counts, const void* image, const double* Ns, int B, int M, int extra, int max_iter,
                                                  double gtol, typename MleArgs<GENERIC>::type pv0, EstOut rho, int32_t* __restrict__ nit_out,
                                                  int32_t* __restrict__ nfev_out, double* __restrict__ fun_out,
                                                  int32_t* __restrict__ status_out, const double* __restrict__ ws_x,
                                                  const double* __restrict__ ws_g, const double* __restrict__ ws_f,
                                                  const int32_t* __restrict__ ws_active, double* __restrict__ pairs) {
  using S = Small<NQ>;
  constexpr int D = S::D;
  bool live;
  const int b = S::trial_index(B, &live);
  const bool mine = live && ws_active[b] != 0;
  if (!__syncthreads_or(mine)) return;  // nothing left to iterate in this workgroup
  extern __shared__ __attribute__((aligned(16))) double smem[];
  std::conditional_t<GENERIC, typename S::Ctx, typename S::template CtxSV<0>> c;  // (no lane tables: CtxSV)
  const int bb = live ? b : B - 1;
  const auto pv = mle_front(pv0, image, Ns, M, extra);
  if constexpr (GENERIC) {
    S::make_ctx(c, smem, pv);
    S::load_freq(c, counts + (size_t)bb * pv.M);
  } else {
    // (behind the ws_active vote: a workgroup with nothing to iterate reads no counts)
    typename S::Prefetch pf;
    S::prefetch_counts(pf, counts + (size_t)bb * pv.M, pv);
    S::take_coefs(c, pv);
    S::make_ctx(c, smem, pv, pf);
    S::load_freq(c, pf);
  }
  // inactive trials of a live wave idle through the loop on dummy finite values
  const double xk = mine ? ws_x[(size_t)b * D + c.l] : (c.l < S::d ? 1.0 : 0.0);
  const double gk = mine ? ws_g[(size_t)b * D + c.l] : 0.0;
  const double fk = mine ? ws_f[b] : 0.0;
  // n = 3: two-loop form (the 64 x 64 inverse Hessian would cost 128 VGPRs per lane); n = 1, 2: H is 4 / 16 doubles
  // per lane and stays in registers
  if constexpr (NQ == 3)
    bfgs_iterate_2l<NQ>(c, mine, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out, pairs);
  else
    bfgs_iterate<NQ>(c, mine, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out);
}

constexpr int kFusedLdsPairs = 24;  // (s, y) pairs of k_mle_fused<3> kept in LDS: 24 KB per trial, 4 trials per workgroup
// ... and of k_mle_fused_hw<3>, whose workgroup also holds a scratch per twin wavefront: 16 KB per trial.  (Where a pair
// lives changes no bit of the iteration.)
constexpr int kFusedHwLdsPairs = 16;

// a10 in ONE launch, for batches small enough that its 256-VGPR footprint (two waves per SIMD) is no
// handicap: start point, first evaluation and -- for the waves that still hold an open trial -- the BFGS
// loop.  Saves the second launch (2.5-4 us when nothing iterates, ~10 % of a 1000-trial step).
// HW (k_mle_fused_hw, n = 3, 'lin' start): launched with blocks of 256 x 2 threads.  threadIdx.y = 0 are the four
// trial wavefronts, exactly as without HW; threadIdx.y = 1 are their twins (Small::HelperLink), wavefront 4 + t on
// the SIMD of wavefront t and with the same threadIdx.x, hence the same trial.  A twin runs the same prologue on the
// same counts with a scratch of its own (make_ctx<.., TWIN>) and parts from the trial's wave behind lin_invert.
template <int NQ, bool GENERIC, bool HW = false>
__device__ __forceinline__ void mle_fused_body(const typename MleArgs<GENERIC>::type& pv, const int64_t* __restrict__ counts, int B, int init,
                                               int max_iter, double gtol, EstOut rho,
                                               int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                               double* __restrict__ fun_out, int32_t* __restrict__ status_out,
                                               double* __restrict__ pairs) {
  using S = Small<NQ>;
  constexpr int D = S::D, G = S::G, d = S::d;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // (one wavefront per SIMD: the specialised context keeps its lane tables decoded in registers)
  using Ctx = std::conditional_t<GENERIC, typename S::Ctx, typename S::template CtxSV<2>>;
  std::conditional_t<HW, typename S::template WithHelper<Ctx>, Ctx> c;
  [[maybe_unused]] typename S::HelperLink link;
  [[maybe_unused]] typename S::LateX late{false, 0.0, 0};
  [[maybe_unused]] int twin = 0;               // HW: this wavefront is a twin (wave-uniform)
  [[maybe_unused]] double* trial_sm = nullptr;  // HW: the scratch of the trial (a twin's own is c.sm)
  // The trial's loads first: nothing but its index stands in front of them (a lone wave issues ~one instruction per 7
  // clocks, and the counts are a cold read).  The twin set-up follows in their shadow.
  bool live;
  const int b = S::trial_index(B, &live);
  const int bb = live ? b : B - 1;
  typename S::Prefetch pf;
  S::prefetch_counts(pf, counts + (size_t)bb * pv.M, pv);
  if constexpr (!GENERIC) S::take_coefs(c, pv);
  if constexpr (HW) {
    static_assert(NQ == 3, "one trial per wavefront");
    static_assert(S::HelperLink::doubles() <= kFusedHwLdsPairs * 2 * D, "the hand-off lives in the LDS pair store");
    int r1 = 6;  // the product POVM's one-qubit rows (the generic body is launched with HW only for a product POVM)
    if constexpr (GENERIC) r1 = pv.pr.R1;
    const int per_trial = S::trial_doubles(pv.M, r1);
    trial_sm = smem + S::table_doubles(pv.M, r1) + (threadIdx.x >> 6) * (per_trial + pv.extra);
    link.base = trial_sm + per_trial + LineSearch::SLOTS + 2 * max_iter;  // TwoLoop::lp
    twin = __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    link.pending = 0;
    if (!twin) link.reset();  // (in front of the workgroup barrier of make_ctx: the twin finds its words set up)
    // The twin is the younger wave of its SIMD and loses the arbitration by age, and it carries the chain the launch
    // waits for (a clipped trial's prologue, lift and evaluation); the older wave has thousands of clocks to spare in
    // every class.  Once, for the whole kernel.  (Measured: profiles/mle_twin_wave_headline_ab.txt.)
    if (twin) __builtin_amdgcn_s_setprio(1);
    c.link = &link;
    c.xtra = trial_sm + per_trial;
    c.late = &late;
  }
  bool shots_ok;
  if constexpr (GENERIC) {
    S::template make_ctx<HW>(c, smem, pv, twin);
    QT_STAMP(0);
    shots_ok = S::load_freq(c, counts + (size_t)bb * pv.M, &pf);
  } else {
    S::template make_ctx<true, HW>(c, smem, pv, pf, twin);
    QT_STAMP(0);
    shots_ok = S::load_freq(c, pf);
  }
  QT_STAMP(1);
  int ok;
  double xk;
  typename S::StartPoint sp;
  [[maybe_unused]] cd lin;
  if (init == 0) {
    double bl;
    lin = S::lin_invert(c, bl);
    QT_STAMP(2);
    // one wave per SIMD: the speculative inverse rides along in the sweep (cholesky_param<SPEC>); HW: the twin
    // wavefront, which holds the same `lin`, speculates, through the whole lift, and the sweep here is the plain one
    bool feasible = false;
    if constexpr (HW) {
      if (twin) {
        // lifted, claimed and published: the matrix stays in these registers and this wave goes on as the trial
        if (!S::twin_lift(c, link, lin, sp.rho)) {
          S::HelperLink::publish(link.gone(), 1);
          return;
        }
        sp.lscale = 1.0;
        link.pending = 1;
        feasible = true;
      }
    }
    if (!feasible) sp.rho = S::template make_feasible<!HW>(c, lin, &xk, &ok, &sp.lscale);
    if constexpr (HW) {
      if (!twin && __builtin_amdgcn_readfirstlane(link.pending)) {
        // the twin owns the trial from here: factorise its matrix for it and leave, writing no output
        int r1 = 6;
        if constexpr (GENERIC) r1 = pv.pr.R1;
        double* twin_sm = smem + S::twin_offset(pv.M, r1, pv.extra) + (threadIdx.x >> 6) * S::trial_doubles(pv.M, r1);
        S::sweep_for(c, link, sp.rho, reinterpret_cast<cd*>(twin_sm + S::oB));
        S::HelperLink::publish(link.gone(), 1);
        return;
      }
    }
  } else {
    sp.rho = cd{c.i == c.j ? 1.0 / d : 0.0, 0.0};
    sp.lscale = 1.0;
    xk = S::cholesky_param(c, sp.rho, ok);
  }
  QT_STAMP(8);
  // A trial that stops at iteration 0 returns sp.rho, and every wave that gets here owns its trial (the other wave of a
  // twin pair has left above): the matrix and the scalars of the common case leave NOW, so that their write latency
  // lies beside the evaluation and not behind the last instruction of the launch's slowest wave.  Behind the
  // evaluation the wave writes only what differs (mle_early_scalars_final; the matrix if a fallback replaced it).  A
  // trial that iterates is written again by the BFGS loop: the same lanes and addresses, later in program order.
  [[maybe_unused]] bool early_rho = false, early_scalars = false;  // wave-uniform
  if constexpr (kEarlyOutputs) {
    S::emit_rho(c, rho, b, live, sp.rho);
    early_rho = true;
    early_scalars = fun_out == nullptr;
    if (early_scalars && live && c.l == 0) store_trial(b, 0, 1, 0.0, TRIAL_OK, nit_out, nfev_out, nullptr, status_out);
  }
  double fk, gk;
  cd rho_l;
  [[maybe_unused]] typename S::DeferredValue dv;
  bool evaluate = true;
  if constexpr (HW) {
    if (__builtin_amdgcn_readfirstlane(link.pending)) {
      // the front of the evaluation beside the helper's factorisation of sp.rho (its lift); x arrives where Tr is formed
      if constexpr (GENERIC) S::template nll_grad<false, decltype(c), true>(c, 0.0, fk, gk, &rho_l, true, &sp);
      else S::template nll_grad<true, decltype(c), true>(c, 0.0, fk, gk, &rho_l, true, &sp, &dv);
      xk = late.x;
      ok = late.ok;
      // Nothing came, or the short cut left something non-positive behind (make_feasible): the serial path, as
      // without a helper, and the evaluation again from the top.  (One trial per wave: both facts are wave-uniform.)
      const bool got = __builtin_amdgcn_readfirstlane((int)late.got) != 0;
      if (!got) xk = S::cholesky_param(c, sp.rho, ok);
      ok = __builtin_amdgcn_readfirstlane(ok);
      evaluate = !got || !ok;
      if (!ok) {
        sp.rho = S::psd_project(c, lin, 1e-15);
        xk = S::cholesky_param(c, sp.rho, ok);
        early_rho = false;  // (the matrix stored above is not the one this trial returns)
      }
    }
  }
  if (evaluate) {
    if constexpr (GENERIC) S::nll_grad(c, xk, fk, gk, &rho_l, true, &sp);
    else S::template nll_grad<true>(c, xk, fk, gk, &rho_l, true, &sp, &dv);
  }
  double gnorm;
  bool iterate;
  if constexpr (kStartBallots<NQ, GENERIC>) {
    bool above;
    gnorm = start_norm_ballots<G>(gk, gtol, above);
    QT_STAMP(9);
    iterate = live && shots_ok && ok && above && (0 < max_iter);
  } else {
    gnorm = gmax<G>(fabs(gk));
    QT_STAMP(9);
    iterate = live && shots_ok && ok && (gnorm > gtol) && (0 < max_iter);
  }
  if constexpr (!GENERIC) fk = S::value_if_needed(c, dv, iterate || fun_out != nullptr);
  // (trials that iterate are written at the end of the loop)
  if constexpr (kEarlyOutputs) {
    S::emit_dist(c, rho, b, live && !iterate, rho_l);
    if (!early_rho) S::emit_rho(c, rho, b, live && !iterate, rho_l);
  } else {
    S::emit(c, rho, b, live && !iterate, rho_l);
  }
  const bool xnan = group_any<G>(xk != xk);
  const int status = mle_start_status(shots_ok, ok, iterate, max_iter, gnorm, fk, xnan);
  const bool stored = early_scalars && mle_early_scalars_final(shots_ok, ok, iterate, max_iter, gnorm, fk, xnan, fun_out != nullptr);
  if (live && !iterate && c.l == 0 && !stored) store_trial(b, 0, ok ? 1 : 0, fk, status, nit_out, nfev_out, fun_out, status_out);
  QT_STAMP(10);
  if (!__any(iterate)) return;  // per wave
  if (!iterate) {                // finite dummies for the groups of this wave that are already done
    xk = (c.l < d) ? 1.0 : 0.0;
    gk = 0.0;
    fk = 0.0;
  }
  // n = 3: two-loop form, the first kFusedLdsPairs (s, y) pairs in LDS (the 64 x 64 inverse Hessian took 128 VGPRs per lane
  // and ~460 AGPR moves per iteration); n = 1, 2: the 4 / 16-entry Hessian rows stay in registers
  if constexpr (HW) link.await_gone();  // the hand-off region is the front of the LDS pair store
  if constexpr (NQ == 3)
    bfgs_iterate_2l<NQ, HW ? kFusedHwLdsPairs : kFusedLdsPairs>(c, iterate, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out,
                                              status_out, pairs);
  else
    bfgs_iterate<NQ>(c, iterate, xk, gk, fk, b, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out);
}

// Two entry points over the same body: the fully mixed start (`init = 'mixed'`: every trial iterates, ~10x the duration)
// runs under its own kernel name, so that a profiler's per-kernel average of k_mle_fused is the average of the
// 'lin'-start launches (bench.py's timed steps) and not a mixture with the iterating side measurements.
template <int NQ, bool GENERIC>
__global__ void __launch_bounds__(256) k_mle_fused(const int64_t* __restrict__ counts, const void* image, const double* Ns, int B, int M, int extra, int max_iter,
                                                   double gtol, typename MleArgs<GENERIC>::type pv, EstOut rho, int32_t* __restrict__ nit_out,
                                                   int32_t* __restrict__ nfev_out, double* __restrict__ fun_out,
                                                   int32_t* __restrict__ status_out, double* __restrict__ pairs) {
  mle_fused_body<NQ, GENERIC>(mle_front(pv, image, Ns, M, extra), counts, B, 0, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out, pairs);
}
template <int NQ, bool GENERIC>
__global__ void __launch_bounds__(256) k_mle_fused_mixed(const int64_t* __restrict__ counts, const void* image, const double* Ns, int B, int M, int extra,
                                                         int max_iter, double gtol, typename MleArgs<GENERIC>::type pv, EstOut rho,
                                                         int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                                         double* __restrict__ fun_out, int32_t* __restrict__ status_out,
                                                         double* __restrict__ pairs) {
  mle_fused_body<NQ, GENERIC>(mle_front(pv, image, Ns, M, extra), counts, B, 1, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out, pairs);
}

// The 'lin' start with a twin wavefront per trial (mle_fused_body<.., HW>): blocks of 256 x 2 threads, the grid of
// k_mle_fused, its LDS layout with kFusedHwLdsPairs pairs and the twins' scratches behind it (Small::lds_bytes_twin).
// Two waves per SIMD: the 256 registers of the body are what a wave can have.
template <int NQ, bool GENERIC>
__global__ void __launch_bounds__(512) k_mle_fused_hw(const int64_t* __restrict__ counts, const void* image, const double* Ns, int B, int M, int extra, int max_iter,
                                                      double gtol, typename MleArgs<GENERIC>::type pv, EstOut rho, int32_t* __restrict__ nit_out,
                                                      int32_t* __restrict__ nfev_out, double* __restrict__ fun_out,
                                                      int32_t* __restrict__ status_out, double* __restrict__ pairs) {
  mle_fused_body<NQ, GENERIC, true>(mle_front(pv, image, Ns, M, extra), counts, B, 0, max_iter, gtol, rho, nit_out, nfev_out, fun_out, status_out, pairs);
}

}  // namespace qt
