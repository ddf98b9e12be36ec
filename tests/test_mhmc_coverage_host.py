"""Host: the chain coverage study's surface without a GPU -- the two C entries are exported and declared, the argument
errors of metrics.get_CL_list_state_mhmc come before any GPU use, and the host instantiation of the chain's random
numbers (qt_sampler::mhmc_draw through tests/host/mhmc_draws_host.cpp) is the stated function of the Philox words."""
import ctypes

import numpy as np
import pytest

import mhmc_coverage_cases as cases
from quantpy_amd import _capi, metrics

ENTRIES = ("qt_mhmc_draws", "qt_mhmc_state_hits")


def test_library_exports_and_capi_declares_the_entries():
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in ENTRIES:
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert len(_capi.SIGNATURES["qt_mhmc_draws"][1]) == 9
    assert len(_capi.SIGNATURES["qt_mhmc_state_hits"][1]) == 16


def test_argument_errors_before_any_gpu_use():
    fn = metrics.get_CL_list_state_mhmc  # (the state is never looked at: these come in front of everything else)
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


def test_refusal_of_the_interval_argument_names_the_study():
    with pytest.raises(NotImplementedError, match="mhmc.*get_CL_list_state_mhmc"):
        metrics.get_CL_list_state(None, interval="mhmc")


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return cases.build_host_draws(tmp_path_factory.mktemp("mhmc_draws"))


def _philox(ctr, key):
    out = np.zeros(4, dtype=np.uint32)
    _capi.load().qt_philox4x32_10(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
    return out


# (seed, first chain, chains, first step, steps): low and high words of seed and chain, steps next to the 2^32 - 2 limit
DRAW_CASES = [(7, 0, 3, 0, 4), (0xDEADBEEF12345678, (1 << 32) + 5, 2, 1000, 3), (2**64 - 1, 2**40, 1, 2**32 - 5, 3)]


@pytest.mark.parametrize("dim", [4, 16, 64])
@pytest.mark.parametrize("case", DRAW_CASES)
def test_host_draws_are_the_stated_function_of_the_philox_words(host_draws, case, dim):
    """Uniforms: uniform53 of words 0, 1 of block D/2 at counter {q, chain low, chain high, 1 + step}, bit for bit.
    Increments: NumPy's Box-Muller on uniform53 of the words of block q, to 1e-13 absolute: |r| <= 8.6, the rounding of
    2 pi u2 contributes <= 6.3 eps and the libm functions a few ulp, below 1e-14 in all."""
    seed, c0, chains, s0, steps = case
    deltas, uniforms = host_draws(seed, c0, chains, s0, steps, dim)
    for c in range(chains):
        for t in range(steps):
            u1, u2, u = cases.defined_draws(_philox, seed, c0 + c, s0 + t, dim)
            assert uniforms[c, t] == u and 0.0 <= u < 1.0
            assert np.abs(deltas[c, t] - cases.box_muller(u1, u2)).max() < 1e-13
    # nothing but the global indices enters: a sub-block called on its own is the same table
    one_d, one_u = host_draws(seed, c0 + chains - 1, 1, s0 + 1, steps - 1, dim)
    assert np.array_equal(one_d[0], deltas[-1, 1:]) and np.array_equal(one_u[0], uniforms[-1, 1:])


def test_host_draws_look_like_standard_normals_and_uniforms(host_draws):
    """A coarse sanity check of the distribution (the definition above is what is pinned): 64 000 increments with mean
    and variance within five standard errors of 0 and 1, the uniforms' mean within five of 1/2."""
    deltas, uniforms = host_draws(12345, 0, 10, 0, 100, 64)
    n = deltas.size
    assert abs(deltas.mean()) < 5 / np.sqrt(n)
    assert abs(deltas.var() - 1.0) < 5 * np.sqrt(2.0 / n)
    assert abs(uniforms.mean() - 0.5) < 5 / np.sqrt(12 * uniforms.size)
