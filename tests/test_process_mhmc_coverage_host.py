"""Host: the surface of the process chain coverage study without a GPU -- the two C entries are exported and declared, the
argument errors of metrics.get_CL_list_channel_mhmc come before any GPU use, the refusal of
get_CL_list_channel(interval='mhmc') names the study, and the host instantiation of the chain's random numbers
(qt_sampler::mhmc_draw through tests/host/mhmc_draws_host.cpp) at the vector lengths of a Choi vector, 16 and 256, is the
stated function of the Philox words, with the uniform at block D^2 / 2."""
import ctypes

import numpy as np
import pytest

import mhmc_coverage_cases as draws_cases
import process_mhmc_coverage_cases as cases
from quantpy_amd import _capi, metrics

ENTRIES = ("qt_mhmc_process_draws", "qt_mhmc_process_hits")


def test_library_exports_and_capi_declares_the_entries():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_capi.SIGNATURES["qt_mhmc_process_draws"][1]) == 9
    assert len(_capi.SIGNATURES["qt_mhmc_process_hits"][1]) == 16


def test_argument_errors_before_any_gpu_use():
    fn = metrics.get_CL_list_channel_mhmc  # (the channel is never looked at: these come in front of everything else)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_iter=0)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_points=0)
    with pytest.raises(ValueError, match="sampler"):
        fn(None, sampler="sobol")
    with pytest.raises(ValueError, match="thinning"):
        fn(None, thinning=0)
    with pytest.raises(ValueError, match="burn_steps"):
        fn(None, burn_steps=-1)
    with pytest.raises(ValueError, match="2\\^32"):
        fn(None, n_points=2**20, thinning=2**12)


def test_three_qubit_channel_is_refused_before_the_engine_is_touched(monkeypatch):
    import quantpy_amd as qp
    from quantpy_amd.tomography.process import ProcessTomograph

    def no_tomograph(*a, **k):
        raise AssertionError("the refusal must come before the tomograph is built")

    monkeypatch.setattr(ProcessTomograph, "__init__", no_tomograph)
    monkeypatch.setattr(ProcessTomograph, "_engine", no_tomograph)
    with pytest.raises(NotImplementedError, match="one and two qubits"):
        metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1)


def test_refusals_of_the_interval_argument_name_the_studies():
    with pytest.raises(NotImplementedError, match="mhmc.*get_CL_list_channel_mhmc"):
        metrics.get_CL_list_channel(None, interval="mhmc")
    with pytest.raises(NotImplementedError, match="mhmc.*get_CL_list_state_mhmc"):
        metrics.get_CL_list_state(None, interval="mhmc")


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return cases.build_host_draws(tmp_path_factory.mktemp("process_mhmc_draws"))


def _philox(ctr, key):
    out = np.zeros(4, dtype=np.uint32)
    _capi.load().qt_philox4x32_10(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
    return out


# (seed, first chain, chains, first step, steps): low and high words of seed and chain, steps next to the 2^32 - 2 limit
DRAW_CASES = [(7, 0, 2, 0, 3), (0xDEADBEEF12345678, (1 << 32) + 5, 2, 1000, 2), (2**64 - 1, 2**40, 1, 2**32 - 5, 3)]


@pytest.mark.parametrize("dim", [16, 256])
@pytest.mark.parametrize("case", DRAW_CASES)
def test_host_draws_are_the_stated_function_of_the_philox_words(host_draws, case, dim):
    """Uniforms: uniform53 of words 0, 1 of block D^2 / 2 at counter {D^2 / 2, chain low, chain high, 1 + step}, bit for
    bit.  Increments: NumPy's Box-Muller on uniform53 of the words of block q, to 1e-13 absolute (|r| <= 8.6, the rounding
    of 2 pi u2 contributes <= 6.3 eps and the libm functions a few ulp: below 1e-14 in all)."""
    seed, c0, chains, s0, steps = case
    deltas, uniforms = host_draws(seed, c0, chains, s0, steps, dim)
    assert deltas.shape == (chains, steps, dim)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    for c in range(chains):
        for t in range(steps):
            u1, u2, u = draws_cases.defined_draws(_philox, seed, c0 + c, s0 + t, dim)
            assert len(u1) == dim // 2
            assert uniforms[c, t] == u and 0.0 <= u < 1.0
            assert np.abs(deltas[c, t] - draws_cases.box_muller(u1, u2)).max() < 1e-13
            # the uniform's block, stated once more without the helper: counter word 0 = D^2 / 2
            chain = c0 + c
            w = _philox(np.array([dim // 2, chain & 0xFFFFFFFF, chain >> 32, 1 + s0 + t], dtype=np.uint32), key)
            assert uniforms[c, t] == draws_cases.u53(w[0], w[1])
    # nothing but the global indices enters: a sub-block called on its own is the same table
    one_d, one_u = host_draws(seed, c0 + chains - 1, 1, s0 + 1, steps - 1, dim)
    assert np.array_equal(one_d[0], deltas[-1, 1:]) and np.array_equal(one_u[0], uniforms[-1, 1:])


def test_state_and_process_chains_of_one_key_share_their_leading_blocks(host_draws):
    """What include/qtomo.h warns of: under one (seed, chain) the increments of a state chain (vector length 16) are the
    first 16 of the process chain's 256, and its uniform is the u1 of the process chain's block 8."""
    short_d, short_u = host_draws(99, 3, 1, 5, 2, 16)
    long_d, _ = host_draws(99, 3, 1, 5, 2, 256)
    assert np.array_equal(short_d, long_d[..., :16])
    u1, _, _ = draws_cases.defined_draws(_philox, 99, 3, 5, 256)
    assert short_u[0, 0] == u1[8]
