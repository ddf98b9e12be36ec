"""Host: the level rule of the coverage studies (quantpy_amd.metrics.levels_from_hits against the reference's own lines,
metrics.py:140-144, on a sorted raw sample) and the argument errors that get_CL_list_state / get_CL_list_channel raise
before anything touches the GPU."""
import numpy as np
import pytest

from quantpy_amd import metrics


def _reference_level(delta, dist):
    """metrics.py:140-144 with `distances` the sorted raw sample and CLs = np.linspace(0, 1, n_points)."""
    distances, cls = np.sort(dist), np.linspace(0, 1, len(dist))
    with np.errstate(invalid="ignore"):
        inside = np.where(delta > distances)[0]
    return 0 if len(inside) == 0 else cls[inside[-1]]


def _hits(delta, dist):
    with np.errstate(invalid="ignore"):
        return int((delta > dist).sum())


def _samples():
    g = np.random.default_rng(5)
    out = []
    for n in (1, 2, 5, 17, 100):
        dist = g.random(n)
        out.append((0.5, dist))
        out.append((-1.0, dist))                    # everything above
        out.append((2.0, dist))                     # everything below
        tied = dist.copy()
        tied[g.integers(0, n, size=max(1, n // 3))] = 0.5
        out.append((0.5, tied))                     # ties with delta do not count (strict comparison)
        holes = tied.copy()
        holes[g.integers(0, n, size=max(1, n // 4))] = np.nan
        out.append((0.5, holes))                    # NaN is sorted last and never below delta
        out.append((0.5, np.full(n, np.nan)))
        out.append((0.0, np.where(g.random(n) < 0.5, 0.0, -0.0)))  # both zeros equal delta = 0
    return out


@pytest.mark.parametrize("case", range(len(_samples())))
def test_levels_from_hits_is_the_reference_rule(case):
    delta, dist = _samples()[case]
    got = metrics.levels_from_hits(np.array([_hits(delta, dist)]), len(dist))
    assert got.shape == (1,) and got[0] == _reference_level(delta, dist)


def test_levels_from_hits_vectorised():
    n = 11
    hits = np.arange(n + 1)
    want = np.concatenate([[0.0], np.linspace(0, 1, n)])
    assert np.array_equal(metrics.levels_from_hits(hits, n), want)


@pytest.mark.parametrize("fn", [metrics.get_CL_list_state, metrics.get_CL_list_channel])
def test_argument_errors_before_any_gpu_use(fn):
    # (the first argument is never looked at: these are raised in front of everything else)
    with pytest.raises(ValueError, match="Incorrect value for argument `interval`"):
        fn(None, interval="bayes")
    with pytest.raises(NotImplementedError, match="mhmc"):
        fn(None, interval="mhmc")
    with pytest.raises(NotImplementedError, match="Hilbert-Schmidt"):
        fn(None, dst="trace")
    with pytest.raises(NotImplementedError, match="Hilbert-Schmidt"):
        fn(None, dst="if")
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_iter=0)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_points=0)
    with pytest.raises(ValueError, match="sampler"):
        fn(None, sampler="sobol")


def test_boot_argument_errors():
    with pytest.raises(NotImplementedError, match="method_boot"):
        metrics.get_CL_list_state(None, interval="boot", method_boot="mle-constr")
    with pytest.raises(NotImplementedError, match="Hilbert-Schmidt"):
        metrics.get_CL_list_state(None, interval="boot", dst="trace")
    with pytest.raises(NotImplementedError, match="boot"):
        metrics.get_CL_list_channel(None, interval="boot")


def test_module_is_exported():
    import quantpy_amd as qp

    assert qp.metrics is metrics
