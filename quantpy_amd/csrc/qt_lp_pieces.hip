// qt_lp_pieces.hip -- k_lp_pieces, the kernel of the test and diagnosis entry qt_lp_pieces, and its launcher.
//
// A translation unit of its own, so that the device code of k_lp_ineq, k_lp_ineq_large and k_lp_ineq_xl in qtomo.hip
// does not depend on it: in one unit the new callers of the out-of-line primitives (lp_normal, lg_normal, lg_solve)
// changed those functions and, through their register use, all three kernels (scripts/isa_identity.py,
// profiles/lp_pieces_isa_identity.txt).  The primitives here are compiled from the same headers.
#define QT_LP_PRIMITIVES_ONLY  // k_lp_ineq, k_lp_ineq_large and k_lp_ineq_xl are qtomo.hip's
#include "qt_lp_xl.h"

namespace qt {

// qt_lp_pieces: one workgroup runs each primitive of P once, on the caller's vectors, and hands every result out, so
// that a test can hold the normal matrix, its factor, A^T v, A y and the solve against a reference one by one (through a
// whole solve the interior-point method corrects a wrong Newton direction and hides them).  P is built as in k_lp_ineq*
// and only its members are called.  n = N + p1 columns; mode 0 is factor(w, p1), mode 1 full_rank(w) (the host refuses
// p1 with it).  Every output may be null; of `normal` and `factor` (n x n, row-major) only the lower triangle is written;
// `solved` is written only after a factorisation that succeeded.  The LDS block starts as all-ones bytes (NaN), like the
// workspace slice and the outputs, which the host fills before the launch: a primitive that reads an entry of H or of an
// n-vector that nothing wrote hands a NaN on instead of a stale value that happens to fit.
template <class P>
__global__ void __launch_bounds__(kLpNT) k_lp_pieces(const double* __restrict__ A, int M, int N, const double* __restrict__ w,
                                                     const double* __restrict__ vm, const double* __restrict__ vn, int p1,
                                                     int mode, double* __restrict__ normal, double* __restrict__ factor,
                                                     double* __restrict__ u, double* __restrict__ ax,
                                                     double* __restrict__ solved, int32_t* __restrict__ ok,
                                                     double* __restrict__ ws) {
  __shared__ typename P::Shared sh;
  const int t = threadIdx.x, n = N + (p1 ? 1 : 0);
  const bool border = p1 != 0;
  {
    double* all = reinterpret_cast<double*>(&sh);
    for (int e = t; e < (int)(sizeof(sh) / sizeof(double)); e += kLpNT) all[e] = __longlong_as_double(-1LL);
  }
  __syncthreads();
  const P p(A, M, N, ws);
  auto triangle = [&](double* out) {  // the lower triangle of H, as the primitives left it
    for (int e = t; e < n * n; e += kLpNT) {
      const int i = e / n, j = e % n;
      if (j <= i) out[e] = p.h_at(sh, i, j);
    }
    __syncthreads();
  };
  if (u) {  // uniform, like every branch below
    p.colsum(sh, vm, border);
    for (int j = t; j < n; j += kLpNT) u[j] = sh.u[j];
    __syncthreads();
  }
  if (ax) {
    for (int j = t; j < N; j += kLpNT) sh.y[j] = vn[j];
    __syncthreads();
    p.matvec(sh.y);
    for (int i = t; i < M; i += kLpNT) ax[i] = p.av(i, sh.y);
    __syncthreads();
  }
  if (normal) {
    p.normal(sh, w, border);
    triangle(normal);
  }
  if (factor || solved || ok) {
    const bool good = mode ? p.full_rank(sh, w) : p.factor(sh, w, border);
    __syncthreads();
    if (ok && t == 0) *ok = good ? 1 : 0;
    if (factor) triangle(factor);
    if (solved && good) {
      for (int j = t; j < n; j += kLpNT) sh.dy[j] = vn[j];
      __syncthreads();
      p.solve(sh, n, sh.dy);
      __syncthreads();
      for (int j = t; j < n; j += kLpNT) solved[j] = sh.dy[j];
    }
  }
}

// One workgroup of k_lp_pieces<LpSmall / LpLarge / LpXl> (kernel 0 / 1 / 2) on `stream`; the caller (qt_lp_pieces in
// qtomo.hip) has checked the sizes and filled ws (that kernel's ws_doubles(M) doubles) and the outputs.
void lp_pieces_launch(int kernel, hipStream_t stream, const double* A, int M, int N, const double* w, const double* vm,
                      const double* vn, int p1, int mode, double* normal, double* factor, double* u, double* ax,
                      double* solved, int32_t* ok, double* ws) {
  auto* k = kernel == 0 ? k_lp_pieces<LpSmall> : kernel == 1 ? k_lp_pieces<LpLarge> : k_lp_pieces<LpXl>;
  hipLaunchKernelGGL(k, dim3(1), dim3(kLpNT), 0, stream, A, M, N, w, vm, vn, p1, mode, normal, factor, u, ax, solved, ok, ws);
}

}  // namespace qt
