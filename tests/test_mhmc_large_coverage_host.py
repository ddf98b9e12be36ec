"""No GPU: the chain coverage study at n = 4, 5 -- the conditions on the inputs of tests/test_gpu_mhmc_large_coverage.py,
checked on the CPU oracle with the host build of the draws, and the three C entries (qt_mhmc_draws_dim,
qt_mhmc_state_large_hits, qt_mhmc_state_large_metric_hits) as the header declares them and _capi binds them."""
import ctypes
import os
import re

import numpy as np
import pytest

import mhmc_coverage_cases as small
import mhmc_large_coverage_cases as cases
from quantpy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return small.build_host_draws(tmp_path_factory.mktemp("mhmc_draws"))


@pytest.mark.parametrize("n", [4, 5])
def test_inputs_meet_their_conditions_on_the_oracle(oracle, host_draws, n):
    """The unclipped 'lin' estimates are positive definite at SHOTS[n] shots per setting (and not at 1000); at the
    recorded Philox seed every chain rejects the recorded number of post-burn steps -- at least one -- and accepts at
    least one, in both settings."""
    counts, rho = cases.trial_counts(oracle, n)
    eig = cases.smallest_eigenvalues(oracle, n, counts)
    print(f"n={n}: smallest eigenvalues {eig}")
    assert eig.min() > 1e-3
    assert cases.smallest_eigenvalues(oracle, n, cases.trial_counts(oracle, n, 1000)[0]).max() < 0.0
    povm = oracle.measurement_matrix("proj-set", n)
    x0 = [oracle.matrix_to_tril_vec(oracle.lin_estimate(c, povm, physical=False)) for c in counts]
    for setting, (burn, n_points, thinning) in sorted(cases.SETTINGS.items()):
        total = burn + n_points * thinning
        deltas, uniforms = host_draws(cases.DRAW_SEEDS[n], 0, cases.CHAINS, 0, total, 4**n)
        rejected = []
        for c in range(cases.CHAINS):
            acc = oracle.mhmc_state_chain(counts[c], povm, x0[c], deltas[c], uniforms[c], cases.STEP)[1][burn:]
            rejected.append(int(len(acc) - acc.sum()))
            assert 0 < acc.sum() < len(acc), (n, setting, c)
        assert rejected == cases.REJECTED[n, setting], (n, setting, rejected)


def _declaration(header, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", header, re.S | re.M)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]
    return [(a.rsplit(" ", 1)[0].rstrip("* ") + ("*" if "*" in a else ""), a.rsplit(" ", 1)[1].lstrip("*")) for a in args]


_CTYPES = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}


def test_capi_declares_the_three_entries_as_the_header_states_them():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("qt_mhmc_draws_dim", "qt_mhmc_state_large_hits", "qt_mhmc_state_large_metric_hits"):
        decl = _declaration(header, name)
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and hasattr(lib, name)
        want = [ctypes.c_void_p if t.endswith("*") else _CTYPES[t] for t, _ in decl]
        assert argtypes == want, (name, decl)
    names = [a for _, a in _declaration(header, "qt_mhmc_draws_dim")]
    assert names == ["h", "dim", "seed", "first_chain", "C", "first_step", "T", "deltas", "uniforms", "flags"]
    # the argument lists of the n <= 3 entries
    for large, sibling in (("qt_mhmc_state_large_hits", "qt_mhmc_state_hits"),
                           ("qt_mhmc_state_large_metric_hits", "qt_mhmc_state_metric_hits")):
        assert _declaration(header, large) == _declaration(header, sibling)
        assert _capi.SIGNATURES[large] == _capi.SIGNATURES[sibling]
