"""Shared by tests/test_mhmc_coverage_host.py and tests/test_gpu_mhmc_coverage.py: the host build of the chain's random
numbers, their definition restated in NumPy, and the batches of trials the GPU tests run."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOTS = 1000


def build_host_draws(tmp_dir):
    """tests/host/mhmc_draws_host.cpp (qt_sampler::mhmc_draw under g++) as draws(seed, first_chain, C, first_step, T, D)
    -> (deltas (C, T, D), uniforms (C, T))."""
    so = os.path.join(str(tmp_dir), "libmhmc_draws_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "host", "mhmc_draws_host.cpp")])
    lib = ctypes.CDLL(so)
    lib.qt_host_mhmc_draws.restype = None
    lib.qt_host_mhmc_draws.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p]

    def draws(seed, first_chain, chains, first_step, steps, dim):
        deltas, uniforms = np.empty((chains, steps, dim)), np.empty((chains, steps))
        lib.qt_host_mhmc_draws(seed, first_chain, chains, first_step, steps, dim, deltas.ctypes.data, uniforms.ctypes.data)
        return deltas, uniforms

    return draws


def u53(w0, w1):
    """uniform53 on two Philox words: 27 high bits of the first, 26 of the second."""
    return ((int(w0) >> 5) * 67108864.0 + (int(w1) >> 6)) / 9007199254740992.0


def defined_draws(philox, seed, chain, step, dim):
    """The definition: (uniforms u1, u2 of the D/2 Box-Muller blocks, the step's uniform) of global step `step` of global
    chain `chain`, from the words of `philox(ctr, key)` at counters {q, chain low, chain high, 1 + step}."""
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    words = []
    for q in range(dim // 2 + 1):
        ctr = np.array([q, chain & 0xFFFFFFFF, chain >> 32, 1 + step], dtype=np.uint32)
        words.append(philox(ctr, key))
    u1 = np.array([u53(w[0], w[1]) for w in words[:-1]])
    u2 = np.array([u53(w[2], w[3]) for w in words[:-1]])
    return u1, u2, u53(words[-1][0], words[-1][1])


def box_muller(u1, u2):
    """NumPy's Box-Muller on the block uniforms: increments 2q, 2q + 1 = r cos(2 pi u2), r sin(2 pi u2)."""
    r = np.sqrt(-2.0 * np.log(1.0 - u1))
    phi = 6.283185307179586 * u2
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=-1).reshape(-1)


def mixed_ghz(n, weight=0.5):
    """weight * |GHZ><GHZ| + (1 - weight) * 1 / d (n = 1: |+><+|): full rank for weight < 1."""
    d = 2**n
    psi = np.zeros(d, dtype=np.complex128)
    psi[0] = psi[-1] = 1 / np.sqrt(2)
    return weight * np.outer(psi, psi.conj()) + (1 - weight) * np.eye(d) / d


def trial_counts(oracle, n, chains, seed):
    """`chains` experiments on the mixed GHZ state, SHOTS per setting, on np.random's stream from `seed`: every chain its
    own counts.  Returns (counts (C, S, K) int64, the true state)."""
    rho = mixed_ghz(n)
    povm = oracle.measurement_matrix("proj-set", n)
    np.random.seed(seed)
    counts = np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(rho), SHOTS) for _ in range(chains)])
    return counts.astype(np.int64), rho
