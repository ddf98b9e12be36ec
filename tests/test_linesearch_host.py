"""CPU: the scalar line-search state machine (quantpy_amd/csrc/qt_linesearch.h, host build)
against SciPy's own scalar_search_wolfe1 -> scalar_search_wolfe2 chain, i.e. what
_line_search_wolfe12 runs inside scipy BFGS (reference call site state.py:213), on 1-D
functions chosen to hit every branch: clean convergence, bracketing, extrapolation, noisy
functions on which dcsrch gives up (fallback search), and outright failures."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest
from scipy.optimize._linesearch import scalar_search_wolfe1, scalar_search_wolfe2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ls") / "libls_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "host", "linesearch_host.cpp")])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def host_ls(host_lib):
    lib = host_lib
    cb_t = ctypes.CFUNCTYPE(None, ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))
    lib.qt_host_line_search.argtypes = [cb_t, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.qt_host_line_search.restype = ctypes.c_int

    def run(phi, dphi, phi0, old_phi0, derphi0):
        def cb(a, pf, pg):
            pf[0] = phi(a)
            pg[0] = dphi(a)

        stp, f, n, mode = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
        ok = lib.qt_host_line_search(cb_t(cb), phi0, old_phi0, derphi0, ctypes.byref(stp), ctypes.byref(f),
                                     ctypes.byref(n), ctypes.byref(mode))
        return (stp.value if ok else None), f.value, n.value, mode.value

    return run


def scipy_wolfe12(phi, dphi, phi0, old_phi0, derphi0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        stp, phi1, _ = scalar_search_wolfe1(phi, dphi, phi0, old_phi0, derphi0, c1=1e-4, c2=0.9,
                                            amax=1e100, amin=1e-100, xtol=1e-14)
        used = 0
        if stp is None:
            used = 1
            stp, phi1, _, dstar = scalar_search_wolfe2(phi, dphi, phi0, old_phi0, derphi0, 1e-4, 0.9, 1e100)
    return stp, phi1, used


def _functions(rng, n):
    out = []
    for i in range(n):
        kind = i % 9
        a, b, c, e = rng.uniform(0.1, 5), rng.uniform(-3, 3), rng.uniform(0.01, 30), rng.uniform(1e-9, 1e-3)
        if kind == 0:  # convex quadratic, minimum anywhere from 1e-3 to 1e3 steps away
            m = 10 ** rng.uniform(-3, 3)
            out.append((lambda t, a=a, m=m: a * (t - m) ** 2, lambda t, a=a, m=m: 2 * a * (t - m)))
        elif kind == 1:  # quartic with a far minimum: extrapolation phase
            out.append((lambda t, c=c: (t - c) ** 4 - 3 * (t - c), lambda t, c=c: 4 * (t - c) ** 3 - 3))
        elif kind == 2:  # log-barrier like the NLL: blows up at a finite step
            out.append((lambda t, c=c, a=a: -np.log(max(c - t, 1e-300)) - a * t,
                        lambda t, c=c, a=a: 1.0 / max(c - t, 1e-300) - a))
        elif kind == 3:  # oscillating
            out.append((lambda t, a=a, b=b: np.sin(a * t + b) + 0.05 * t * t - 2 * t,
                        lambda t, a=a, b=b: a * np.cos(a * t + b) + 0.1 * t - 2))
        elif kind == 4:  # inconsistent (noisy) derivative: forces warnings / the fallback search
            out.append((lambda t, a=a: a * (t - 1) ** 2 + 1e-3 * np.sin(1e4 * t),
                        lambda t, a=a, e=e: 2 * a * (t - 1) + 0.3 * np.cos(37 * t) * (1 + e)))
        elif kind == 5:  # step discontinuity inside the bracket: dcsrch stops on rounding/xtol warnings
            out.append((lambda t, a=a, c=c: a * (t - 1) ** 2 + 0.5 * (t > 0.3 + 0.01 * c),
                        lambda t, a=a: 2 * a * (t - 1)))
        elif kind == 6:  # derivative that never turns positive although phi rises: no Wolfe point
            out.append((lambda t, a=a: a * t * t - t, lambda t, e=e: -1.0 - e))
        elif kind == 7:  # value noise of the size of the decrease: sufficient-decrease test flickers
            out.append((lambda t, e=e, b=b: -e * t + e * np.sin(977.0 * t + b) + t ** 4,
                        lambda t, e=e: -e + 4 * t ** 3))
        else:  # nearly flat
            out.append((lambda t, e=e: -e * t + e * e * t * t, lambda t, e=e: -e + 2 * e * e * t))
    return out


def test_state_machine_matches_scipy_chain(host_ls):
    rng = np.random.default_rng(123)
    n_fallback = n_fail = n_ok = 0
    for phi, dphi in _functions(rng, 600):
        phi0, derphi0 = phi(0.0), dphi(0.0)
        if not derphi0 < 0:
            phi_, dphi_ = phi, dphi
            phi, dphi = (lambda t, p=phi_: p(-t)), (lambda t, d=dphi_: -d(-t))
            phi0, derphi0 = phi(0.0), dphi(0.0)
        for old in (phi0 + abs(derphi0) / 2, phi0 + rng.uniform(1e-6, 10), phi0 - 1.0):
            ref_stp, ref_phi, used = scipy_wolfe12(phi, dphi, phi0, old, derphi0)
            stp, f, n, mode = host_ls(phi, dphi, phi0, old, derphi0)
            n_fallback += used
            if ref_stp is None:
                n_fail += 1
                assert stp is None
            else:
                n_ok += 1
                assert stp is not None
                assert stp == pytest.approx(ref_stp, rel=1e-12, abs=0), (stp, ref_stp)
                assert f == pytest.approx(ref_phi, rel=1e-12, abs=1e-300)
                assert (mode != 0) == bool(used)
    # the sample must actually exercise the fallback and the failure exits
    assert n_ok > 1000 and n_fallback > 100 and n_fail > 20, (n_ok, n_fallback, n_fail)


def test_non_descent_direction_goes_to_fallback_and_fails(host_ls):
    phi, dphi = (lambda t: (t + 1) ** 2), (lambda t: 2 * (t + 1))
    ref = scipy_wolfe12(phi, dphi, phi(0.0), phi(0.0) + 1, dphi(0.0))
    got = host_ls(phi, dphi, phi(0.0), phi(0.0) + 1, dphi(0.0))
    assert ref[0] is None and got[0] is None


# ---- the scalar rules of _minimize_bfgs around the line search (bfgs_* / mle_start_status in qt_linesearch.h).
# Expected values: scipy/optimize/_optimize.py, _minimize_bfgs (1.8 to 1.15: the same lines), xrtol = 0, with
# warnflag 2 -> 2 (LINESEARCH), 1 -> 3 (MAXITER), 3 -> 4 (NAN).
OK, NOT_PD, LINESEARCH, MAXITER, NAN_, SHOTS = range(6)
nan, inf = float("nan"), float("inf")


@pytest.fixture(scope="module")
def rules(host_lib):
    lib = host_lib
    lib.qt_host_eval_cap.argtypes = [ctypes.c_int]
    lib.qt_host_rho.argtypes, lib.qt_host_rho.restype = [ctypes.c_double], ctypes.c_double
    lib.qt_host_step_exit.argtypes = [ctypes.c_double] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.qt_host_final_status.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 3
    lib.qt_host_start_status.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_int]

    def step_exit(gnorm, gtol, stp, pnorm2, fk, kiter, max_iter):
        status = ctypes.c_int(OK)
        stop = lib.qt_host_step_exit(gnorm, gtol, stp, pnorm2, fk, kiter, max_iter, ctypes.byref(status))
        return bool(stop), status.value

    lib.step_exit = step_exit
    return lib


def test_eval_cap_and_rho(rules):
    assert [rules.qt_host_eval_cap(m) for m in (0, 1, 100)] == [260, 390, 13260]
    # rhok_inv == 0. -> 1000.0, else 1 / rhok_inv
    for ys, want in ((0.0, 1000.0), (-0.0, 1000.0), (2.0, 0.5), (-4.0, -0.25), (5e-324, inf), (inf, 0.0)):
        assert rules.qt_host_rho(ys) == want, ys
    assert np.isnan(rules.qt_host_rho(nan))


# (gnorm, stp, pnorm2, fk, kiter) at gtol = 1e-5, max_iter = 10 -> (stop, status); one block per exit, in SciPy's
# order, each row of a block also armed with every LATER exit it must win against
STEP_TABLE = [
    # 1. gnorm <= gtol: break, warnflag 0
    ((1e-6, 1.0, 1.0, 0.5, 3), (True, OK)),
    ((1e-5, 1.0, 1.0, 0.5, 3), (True, OK)),
    ((0.0, 0.0, 0.0, inf, 10), (True, OK)),
    ((1e-6, 1.0, 1.0, nan, 10), (True, OK)),
    # 2. alpha_k * |pk| <= 0: break, warnflag 0
    ((1.0, 0.0, 1.0, 0.5, 3), (True, OK)),
    ((1.0, 1.0, 0.0, 0.5, 3), (True, OK)),
    ((1.0, -1.0, 1.0, 0.5, 3), (True, OK)),
    ((1.0, 0.0, 1.0, nan, 10), (True, OK)),
    ((nan, 0.0, 1.0, -inf, 10), (True, OK)),
    # 3. not isfinite(fval): warnflag 2 (in front of the iteration cap, and of a NaN norm leaving the loop)
    ((1.0, 1.0, 1.0, inf, 3), (True, LINESEARCH)),
    ((1.0, 1.0, 1.0, -inf, 3), (True, LINESEARCH)),
    ((1.0, 1.0, 1.0, nan, 3), (True, LINESEARCH)),
    ((1.0, 1.0, 1.0, nan, 10), (True, LINESEARCH)),
    ((nan, 1.0, 1.0, inf, 3), (True, LINESEARCH)),
    ((1.0, nan, 1.0, inf, 3), (True, LINESEARCH)),  # (nan <= 0 is false: the xrtol test lets a NaN step through)
    # 4. the loop condition, gnorm > gtol and k < maxiter: leaves with warnflag still 0
    ((1.0, 1.0, 1.0, 0.5, 10), (True, OK)),
    ((1.0, 1.0, 1.0, 0.5, 11), (True, OK)),
    ((nan, 1.0, 1.0, 0.5, 3), (True, OK)),
    ((nan, nan, nan, 0.5, 3), (True, OK)),
    # 5. goes on
    ((1.0, 1.0, 1.0, 0.5, 9), (False, OK)),
    ((inf, 1.0, 1.0, 0.5, 3), (False, OK)),
    ((1.0, 1.0, inf, -1e300, 1), (False, OK)),
    ((1.0, nan, 1.0, 0.5, 3), (False, OK)),
    ((2e-5, 1e-100, 1e-200, 0.0, 3), (False, OK)),
]


def test_step_exit_table(rules):
    for (gnorm, stp, pnorm2, fk, kiter), want in STEP_TABLE:
        assert rules.step_exit(gnorm, 1e-5, stp, pnorm2, fk, kiter, 10) == want, (gnorm, stp, pnorm2, fk, kiter)


def _scipy_after_step(gnorm, gtol, alpha_k, pnorm, fval, k, maxiter):
    """The lines of _minimize_bfgs between `k += 1` and the Hessian update, then its loop condition; the number says
    which exit was taken."""
    if gnorm <= gtol:
        return True, 0, 1
    if alpha_k * pnorm <= 0.0:
        return True, 0, 2
    if not np.isfinite(fval):
        return True, 2, 3
    if not ((gnorm > gtol) and (k < maxiter)):
        return True, 0, 4
    return False, 0, 5


def test_step_exit_special_values(rules):
    special = (0.0, 1e-5, 1.0, nan, inf)
    taken = set()
    for gnorm in special:
        for stp in (-1.0,) + special:
            for pnorm in special:
                for fk in (-inf, -1.0) + special:
                    for kiter, max_iter in ((1, 1), (1, 2), (2, 2), (3, 2)):
                        stop, warnflag, which = _scipy_after_step(gnorm, 1e-5, stp, pnorm, fk, kiter, max_iter)
                        taken.add(which)
                        got = rules.step_exit(gnorm, 1e-5, stp, pnorm * pnorm, fk, kiter, max_iter)
                        assert got == (stop, warnflag), (gnorm, stp, pnorm, fk, kiter, max_iter)
    assert taken == {1, 2, 3, 4, 5}


# (status in the loop, kiter, max_iter, gn, fk, xn) -> status: warnflag 2 stands, then k >= maxiter, then NaN
FINAL_TABLE = [
    ((LINESEARCH, 10, 10, nan, nan, nan), LINESEARCH),
    ((LINESEARCH, 0, 10, 1.0, 0.5, 1.0), LINESEARCH),
    ((OK, 10, 10, 1e-9, 0.5, 1.0), MAXITER),
    ((OK, 10, 10, nan, nan, nan), MAXITER),  # 3 before 4
    ((OK, 11, 10, 1.0, inf, 1.0), MAXITER),
    ((OK, 0, 0, 1.0, 0.5, 1.0), MAXITER),
    ((OK, 9, 10, nan, 0.5, 1.0), NAN_),
    ((OK, 9, 10, 1.0, nan, 1.0), NAN_),
    ((OK, 9, 10, 1.0, 0.5, nan), NAN_),
    ((OK, 9, 10, inf, 0.5, 1.0), OK),  # isnan, not isfinite
    ((OK, 9, 10, 1.0, -inf, inf), OK),
    ((OK, 9, 10, 1e-9, 0.5, 1.0), OK),
]


def test_final_status_table(rules):
    for args, want in FINAL_TABLE:
        assert rules.qt_host_final_status(*args) == want, args


# (shots_ok, ok, iterate, max_iter, gnorm, fk, xnan) -> status of a trial at its start point
START_TABLE = [
    ((0, 0, 0, 0, nan, nan, 1), SHOTS),
    ((0, 1, 1, 10, 1.0, 0.5, 0), SHOTS),
    ((1, 0, 0, 0, nan, nan, 1), NOT_PD),
    ((1, 0, 1, 10, 1.0, 0.5, 0), NOT_PD),
    ((1, 1, 1, 10, 1.0, 0.5, 0), OK),
    ((1, 1, 0, 0, 1.0, 0.5, 0), MAXITER),
    ((1, 1, 0, 0, nan, nan, 1), MAXITER),  # 3 before 4
    ((1, 1, 0, -1, 1e-9, 0.5, 0), MAXITER),
    ((1, 1, 0, 10, nan, 0.5, 0), NAN_),
    ((1, 1, 0, 10, 1e-9, nan, 0), NAN_),
    ((1, 1, 0, 10, 1e-9, 0.5, 1), NAN_),
    ((1, 1, 0, 10, 1e-9, inf, 0), OK),
    ((1, 1, 0, 10, 1e-9, 0.5, 0), OK),
]


def test_start_status_table(rules):
    for args, want in START_TABLE:
        assert rules.qt_host_start_status(*args) == want, args
    # without the shot check and with a factorisation, the start is the final rule at k = 0
    for _, kiter, max_iter, gn, fk, xn in (a for a, _ in FINAL_TABLE if a[0] == OK and a[1] == 0):
        assert rules.qt_host_start_status(1, 1, 0, max_iter, gn, fk, int(xn != xn)) == \
            rules.qt_host_final_status(OK, kiter, max_iter, gn, fk, xn)
