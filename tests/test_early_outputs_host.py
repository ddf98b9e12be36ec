"""CPU: the rule by which the one-launch n <= 3 MLE kernels decide that the scalars they stored in front of a trial's
first evaluation -- nit = 0, nfev = 1, status = TRIAL_OK -- are the trial's final ones (mle_early_scalars_final in
quantpy_amd/csrc/qt_linesearch.h, host build).  It must say "final" exactly when what the kernel would store at the
start point, (0, ok ? 1 : 0, mle_start_status(...)), is that triple and the caller did not ask for the value."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK = 0
EARLY = (0, 1, OK)
nan = float("nan")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("early") / "libearly_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "host", "early_outputs_host.cpp")])
    lib = ctypes.CDLL(out)
    lib.qt_host_start_status.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_int]
    lib.qt_host_early_scalars_final.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 2 + [ctypes.c_int] * 2
    return lib


# (gnorm, fk, xnan): finite, and a NaN in each of the three places mle_start_status looks at
NORMS = [(1e-9, 0.5, 0), (nan, 0.5, 0), (1e-9, nan, 0), (1e-9, 0.5, 1), (nan, nan, 1)]


def test_early_scalars_final_table(rules):
    seen = {True: 0, False: 0}
    for shots_ok, ok, iterate, max_iter, fun in itertools.product((0, 1), (0, 1), (0, 1), (0, 1), (0, 1)):
        for gnorm, fk, xnan in NORMS:
            args = (shots_ok, ok, iterate, max_iter, gnorm, fk, xnan)
            triple = (0, 1 if ok else 0, rules.qt_host_start_status(*args))
            want = triple == EARLY and not fun
            assert bool(rules.qt_host_early_scalars_final(*args, fun)) == want, (args, fun, triple)
            seen[want] += 1
    assert seen[True] > 0 and seen[False] > 0, seen


def test_named_cases(rules):
    """The cases the kernels meet, one by one."""
    f = rules.qt_host_early_scalars_final
    assert f(1, 1, 0, 100, 1e-9, 0.0, 0, 0) == 1   # the common case: stops at iteration 0
    assert f(1, 1, 0, 100, 1e-9, 0.5, 0, 1) == 0   # the value is asked for: store_trial writes it
    assert f(0, 1, 0, 100, 1e-9, 0.0, 0, 0) == 0   # wrong shot total: status 5
    assert f(1, 0, 0, 100, 1e-9, 0.0, 0, 0) == 0   # no factorisation: nfev = 0, status 1
    assert f(1, 1, 0, 0, 1e-9, 0.0, 0, 0) == 0     # max_iter = 0: status 3
    assert f(1, 1, 0, 100, nan, 0.0, 0, 0) == 0    # NaN gradient: status 4
    assert f(1, 1, 0, 100, 1e-9, 0.0, 1, 0) == 0   # NaN parameters: status 4
    assert f(1, 1, 1, 100, 1.0, 0.5, 0, 0) == 1    # iterates: the start triple is the early one (the loop writes its own)
