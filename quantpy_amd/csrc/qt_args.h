// What the estimator kernels of every size take and leave: the POVM as the device sees it (ProductView, PovmView, and
// SpecArgs for the specialised n <= 3 MLE kernels), the shots check, the table of centres a distance is measured to
// (centre_of), where a trial's estimate goes (EstOut) and where the scalars of its MLE result go (store_trial).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qt {

// A POVM that is the n-fold tensor product of a one-qubit table T[R1][4] (every built-in POVM and
// every array with a last axis of 4 -- measurements.py:88-93): the M x D contractions A' b, A'^T r and
// A'^+ f factor into n small ones, qubit by qubit (R1^q 4^(n-q) outputs of 4 or R1 terms each), which
// cuts the FP64 work per evaluation ~8x at n = 3 and removes every global load from the inner loops.
// Intermediate arrays live in the trial's LDS scratch in "R-order": index [r_1 .. r_q][k_(q+1) .. k_n]
// with r = s * K1 + o the row of T.  The (base, selector) of every output is tabulated on the host.
struct ProductView {
  const double* T;      // [R1][4]
  const double* P1T;    // [R1][4]  P1T[r][k] = pinv(T)[k][r]  (used when the shot weights are uniform)
  const double* wrowR;  // [M]  N_s / sum(N) of each row, R-order
  const int* rmap;      // [M]  R-order index -> row m of the (S, K) layout
  const int* rinv;      // [M]  the inverse map: row m of the (S, K) layout -> R-order index
  const int* fwd;       // stage tables of the forward pass, stage 1 .. n concatenated: base | sel << 16
  const int* bwd;       // stage tables of the backward pass, stage n .. 1 concatenated
  int R1;
  int uniform;          // all N_s equal
  double wuni;          // the common weight
  int enabled;
  // A six-row table whose rows 2a, 2a+1 are zero outside columns 0 and a+1 (the six-projector POVMs 'proj-set' and
  // 'proj', and their pseudo-inverses) is "paired": half of every stage's terms are fma(0, x, acc).  The n <= 3
  // stages then skip them (same terms, same order: same bits) and take the coefficients from here instead of LDS.
  int pairedT, pairedP;  // T / pinv(T)^T has that shape and QT_OPT_PAIRED_STAGES is on (n <= 3 only)
  double cT[12], cP[12];  // (u_r, v_r) = (tab[r][0], tab[r][r / 2 + 1]), r = 0 .. 5: the bits of T and P1T
  const int* last;       // [M] stage-n entries of a paired T: in0 | axis << 8 | (4 r + a + 1) << 16
};

struct PovmView {
  const double* Aw;    // [M][D]  shot-weighted A'
  const double* AwT;   // [D][M]
  const double* PinvT; // [M][D]  transpose of the left inverse of A'
  int M;
  ProductView pr;
  double jtol2 = 1e-28;  // Jacobi stops when off-diagonal norm^2 <= jtol2 * Frobenius norm^2
  // shots per setting as registered with qt_set_povm (the weights N_s / sum N inside A' come from these);
  // every trial's own per-setting totals must be proportional to them (state.py:138-141, 194-197: the
  // reference takes the weights from the trial's results) or the trial is flagged QT_TRIAL_SHOTS
  const double* Ns = nullptr;  // [S]
  int S = 0, K = 0;
  double ns_tot = 0.0;
  int extra = 0;  // extra doubles of per-trial LDS behind the scratch (k_mle_bfgs: line-search state + two-loop scalars)
};

// What the specialised MLE kernels (template parameter GENERIC = false, n <= 3) take instead of a PovmView.  They are
// compiled for ONE launch-uniform shape, that of every built-in six-projector run: a product POVM with R1 = 6 rows
// made of three two-outcome settings (so K = d outcomes per setting, M = 6^n <= 4 G rows), both one-qubit tables
// paired, equal shots per setting, the shots check on.  Nothing else of the POVM is read, so nothing else is passed:
// the PovmView is 0x1b8 bytes of kernel arguments, most of them dead on this path and all of them live in SGPRs.
// `image` is built once by qt_set_povm_product, in device memory: the workgroup's LDS table block in its final layout
// (Small::image_chunks(M) 16-byte chunks: the stage-n entries `last`[M], padded to a multiple of four, then T [6][4]
// and pinv(T)^T [6][4]) followed by rinv[M].
struct SpecArgs {
  const void* image;
  const double* Ns;  // [S] registered shots per setting
  double ns_tot, wuni, jtol2;
  int M, extra;
  double cT[12], cP[12];  // ProductView::cT / cP
};
template <bool GENERIC>
struct MleArgs {
  using type = PovmView;
};
template <>
struct MleArgs<false> {
  using type = SpecArgs;
};

// The n <= 3 MLE kernels (qt_mle_small.h) lead with what the first batch of a trial's loads needs, as plain pointers and
// ints in front of the struct: (counts, image, Ns, B, M, extra, max_iter, gtol).  The compiler preloads a kernel's leading
// plain arguments into SGPRs at wave launch (build.py: PRELOAD_FLAGS) and stops at the first aggregate, so the addresses of
// those loads hang on no load of the argument segment: 0.2 us of the 8.9 us headline step (DESIGN 4.1,
// profiles/trial_front_headline_ab.txt).  The struct keeps its fields; mle_front writes the leading values into the
// kernel's copy, and the body reads one struct as before.  A PovmView has no image: the generic launch passes nullptr in
// that slot.
__device__ __forceinline__ SpecArgs mle_front(SpecArgs a, const void* image, const double* Ns, int M, int extra) {
  a.image = image;
  a.Ns = Ns;
  a.M = M;
  a.extra = extra;
  return a;
}
__device__ __forceinline__ PovmView mle_front(PovmView pv, const void*, const double* Ns, int M, int extra) {
  pv.Ns = Ns;
  pv.M = M;
  pv.extra = extra;
  return pv;
}

// t_s / total == N_s / ns_tot, compared as cross products of integer-valued doubles (exact below 2^53; a few
// ulp of slack beyond that -- one stray count out of N_s < 1e14 is still seen)
__device__ __forceinline__ bool shots_match(double t_s, double total, double n_s, double ns_tot) {
  const double a = t_s * ns_tot, b = n_s * total;
  return fabs(a - b) <= 2e-15 * fabs(b);
}

// Where an estimator leaves a trial's result: the density matrix and / or -- the body of the bootstrap loop,
// interval.py:600-609, `dist[i] = dst(point_estimate(...), state)` -- its Hilbert-Schmidt distance (geometry.py:16-20) to
// `centre`.  With `dist` set and `rho` null a resample costs 8 bytes of HBM writes instead of 16 d^2 and no second pass.
// A table of G centres serves the nested bootstrap of the coverage study (metrics.py:125-144), where every trial of the
// study has its own point estimate: the batch is then [resample][trial] and trial b is measured against centre (g0 + b) % G
// (g0: the group of the launch's first trial, for a launch that starts inside the batch).  G == 1 is the single centre and
// takes no modulo.
// Centre (g0 + b) % G of a table of G matrices of dd doubles each.  Defined for every b >= 0.
__device__ __forceinline__ const double* centre_of(const double* centres, int G, int g0, int b, int dd) {
  return G > 1 ? centres + (size_t)((unsigned)(g0 + b) % (unsigned)G) * dd : centres;
}

struct EstOut {
  double* rho;           // [B][d][d][2], or nullptr when only the distance is wanted
  const double* centre;  // [G][d][d][2], read when dist != nullptr
  double* dist;          // [B], or nullptr
  int G = 1;             // centres in the table (launch-uniform)
  int g0 = 0;            // group of trial 0 of this launch, < G
  // The centre of trial b, dd doubles each.  Reduced for every b >= 0, so the lane groups that pad the last workgroup
  // (b >= B, stores masked) read inside the table too.
  __device__ __forceinline__ const double* centre_of(int b, int dd) const {
    return qt::centre_of(centre, G, g0, b, dd);
  }
};

// The scalars of one trial's MLE result (each output is optional), written by the trial's first lane.
__device__ __forceinline__ void store_trial(int b, int nit, int nfev, double fun, int status,
                                            int32_t* __restrict__ nit_out, int32_t* __restrict__ nfev_out,
                                            double* __restrict__ fun_out, int32_t* __restrict__ status_out) {
  if (nit_out) nit_out[b] = nit;
  if (nfev_out) nfev_out[b] = nfev;
  if (fun_out) fun_out[b] = fun;
  if (status_out) status_out[b] = status;
}

}  // namespace qt
