"""A NumPy model of the interior-point iteration of the batched LP kernels (csrc/qt_lp.h, csrc/qt_lp_large.h), for tests:

    minimise c . x  subject to  A x <= b,  x free.

Same phases, steps and stopping tests as the kernels: Mehrotra predictor-corrector on the normal equations
H = A^T diag(z / s) A, phase 1 on min t, A x - t 1 <= b from x = 0 up to the first strictly feasible x, phase 2 from
there with z = mean(s) / s, tolerance 1e-10, at most 100 iterations per phase.

Two safeguards of the factorisation can be switched on.  `pivot_rel` is the large kernel's (kLgPivot): a pivot not
above pivot_rel of its diagonal entry of H is replaced by that entry; a factorisation without such a pivot is the
plain one.  `shift` factors H + shift * diag(H) every time; it is kept because it was tried and dropped: at 1e-12 it
stalled one of the random programs of tests/test_gpu_lp_large.py ((300, 128), the last program) that converges in 18
iterations without any safeguard.  With neither, a non-positive pivot ends the program as NOT_CONVERGED, as in the
small kernel.  LARGE_PIVOT was 1e-13 at first; a pivot just above that can still be rounding noise, and one program in
several hundred of a four-qubit state interval then overflowed in the factor, here as in the kernel; 1e-12 ... 1e-9
solve it.  The model is where a safeguard is tried first; the kernel follows it.  It is not bit-compatible with
the kernels (BLAS sums in another order), only the same algorithm.
"""
import numpy as np

OPTIMAL, INFEASIBLE, UNBOUNDED, NOT_CONVERGED, FEASIBLE = 0, 1, 2, 3, 4  # qt_lp_status; FEASIBLE: phase 1 only
LARGE_PIVOT = 1e-11  # kLgPivot of csrc/qt_lp_large.h
# The constants of phase() below (tol, cap, the 1e-9 Farkas margin, the 1e-8 / -1e10 unbounded test) are those of
# lp_phase in csrc/qt_lp.h (kTol, kLpCap and the literals beside them), the one place where both kernels have them.


def _max_step(x, dx):
    neg = dx < 0
    return np.min(-x[neg] / dx[neg]) if neg.any() else np.inf


def cholesky_replacing(H, rel, trace=None):
    """Right-looking Cholesky of H in which a pivot not above rel * (its diagonal entry of H) is replaced by that entry
    -> (L, number of replaced pivots).  Raises LinAlgError on a diagonal entry that is not positive.  Works in H's
    precision (float64 or longdouble).  trace: a list that receives (pivot / diagonal entry, replaced) per column."""
    n = H.shape[0]
    L = np.tril(H)
    d0 = np.diag(H).copy()
    replaced = 0
    for k in range(n):
        p = L[k, k]
        if not np.isfinite(p) or not d0[k] > 0.0:
            raise np.linalg.LinAlgError("breakdown")
        if trace is not None:
            trace.append((float(p / d0[k]), not p > rel * d0[k]))
        if not p > rel * d0[k]:
            p = d0[k]
            replaced += 1
        L[k, k] = np.sqrt(p)
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    return L, replaced


def phase(A, b, c, y, s, z, p1, shift=0.0, pivot_rel=None, cap=100, tol=1e-10):
    """One phase, in place on y, s, z -> (status, iterations)."""
    M, N = A.shape
    Af = np.hstack([A, -np.ones((M, 1))]) if p1 else A
    amax, bn, cn = np.abs(A).max(), max(1.0, np.abs(b).max()), max(1.0, np.abs(c).max())
    for it in range(cap):
        rp = Af @ y + s - b
        rd = Af.T @ z + c
        gap = s @ z
        mu = gap / M
        pobj = c @ y
        pres = np.abs(rp).max() / max(bn, amax * np.abs(y).sum())
        dres = np.abs(rd).max() / max(cn, amax * z.sum())
        if not np.all(np.isfinite([gap, pres, dres, pobj])):
            return NOT_CONVERGED, it + 1
        if p1 and (A @ y[:N] - b).max() < 0:
            return FEASIBLE, it + 1
        if pres <= tol and dres <= tol and gap <= tol * max(1.0, abs(pobj)):
            return (INFEASIBLE if p1 else OPTIMAL), it + 1
        if p1 and pres <= tol and dres <= tol and pobj - gap > 1e-9 * max(1.0, abs(pobj)):
            return INFEASIBLE, it + 1
        if not p1 and pres <= 1e-8 and pobj < -1e10 * cn * bn:
            return UNBOUNDED, it + 1
        w = z / s
        H = Af.T @ (w[:, None] * Af)
        try:
            if pivot_rel is None:
                L = np.linalg.cholesky(H + shift * np.diag(np.diag(H)))
            else:
                L = cholesky_replacing(H, pivot_rel)[0]
        except np.linalg.LinAlgError:
            return NOT_CONVERGED, it + 1

        def solve(v):
            return np.linalg.solve(L.T, np.linalg.solve(L, v))

        dy = solve(-rd + Af.T @ (z - z * rp / s))
        ds = -rp - Af @ dy
        dz = -z - z * ds / s
        ap, ad = min(1.0, _max_step(s, ds)), min(1.0, _max_step(z, dz))
        muaff = (s + ap * ds) @ (z + ad * dz) / M
        sigma_mu = (muaff / mu) ** 3 * mu
        rsz = s * z + ds * dz - sigma_mu
        dy = solve(-rd + Af.T @ ((rsz - z * rp) / s))
        ds = -rp - Af @ dy
        dz = (-rsz - z * ds) / s
        ap, ad = min(1.0, 0.99 * _max_step(s, ds)), min(1.0, 0.99 * _max_step(z, dz))
        s += ap * ds
        z += ad * dz
        y += ap * dy
    return NOT_CONVERGED, cap


def ipm(A, b, c, shift=0.0, pivot_rel=None):
    """-> (status, objective, iterations of both phases, x); the objective follows the kernels' convention (+inf
    infeasible, -inf unbounded, NaN not converged)."""
    A, b, c = (np.asarray(v, dtype=np.float64) for v in (A, b, c))
    M, N = A.shape
    t0 = max((-b).max(), 0.0) + 1.0
    y = np.zeros(N + 1)
    y[N] = t0
    s = b + t0
    z = np.full(M, 1.0 / M)
    c1 = np.zeros(N + 1)
    c1[N] = 1.0
    st, iters = phase(A, b, c1, y, s, z, True, shift, pivot_rel)
    x = y[:N].copy()
    if st == FEASIBLE:
        s = b - A @ x
        z = s.mean() / s
        st, i2 = phase(A, b, c, x, s, z, False, shift, pivot_rel)
        iters += i2
    obj = {OPTIMAL: c @ x, INFEASIBLE: np.inf, UNBOUNDED: -np.inf}.get(st, np.nan)
    return st, obj, iters, x
