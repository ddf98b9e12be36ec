"""GPU: the Python paths that choose a library entry by size -- Engine.metric_dist, Engine.distance,
Engine.mhmc_state_hits -- return the bits of the raw entries they stand for, and the three draws entries, which share one
body, give one table at one vector length.

Every comparison is np.array_equal: both sides run the same kernels on the same arrays (qt_metric_dist_group_batch is
qt_metric_dist_dim at the handle's own size, qt_hs_dist_batch is qt_hs_dist_dim there), so there is no tolerance to
derive.  Matrices are random density matrices (Hermitian, positive definite: no NaN on either side)."""
import numpy as np
import pytest

import mhmc_coverage_cases as small
import mhmc_large_coverage_cases as large

pytestmark = pytest.mark.gpu

METRICS = ["trace", "if"]


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _density(rng, shape, dim):
    a = rng.standard_normal(shape + (dim, dim)) + 1j * rng.standard_normal(shape + (dim, dim))
    rho = a @ np.conj(np.swapaxes(a, -1, -2))
    return np.ascontiguousarray(rho / np.trace(rho, axis1=-2, axis2=-1)[..., None, None])


def _p(a):
    return None if a is None else a.ctypes.data


# ---- 1, 2. metric distances ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_metric_dist_is_the_group_entry_at_the_engines_own_size(qp, n, metric):
    from quantpy_amd import _capi

    eng = qp.get_engine(n)
    rng = np.random.default_rng(40 + n)
    rho, cen = _density(rng, (5,), 2**n), _density(rng, (2,), 2**n)
    want = np.full(5, np.nan)
    rc = eng.lib.qt_metric_dist_group_batch(eng._h, eng._METRICS[metric], _p(rho), 5, _p(cen), 2, 1, _p(want), _capi.QT_HOST_PTR)
    assert rc == 0 and np.all(np.isfinite(want)) and want.max() > 1e-6
    assert np.array_equal(eng.metric_dist(rho, cen, metric, g0=1), want)
    assert np.array_equal(eng.distance(rho, cen, metric, g0=1), want)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [16, 32])
def test_metric_dist_is_the_dim_entry_at_a_foreign_size(qp, dim, metric):
    from quantpy_amd import _capi

    eng = qp.get_engine(1)
    rng = np.random.default_rng(dim)
    rho, cen = _density(rng, (3,), dim), _density(rng, (), dim)
    want = np.full(3, np.nan)
    rc = eng.lib.qt_metric_dist_dim(eng._h, eng._METRICS[metric], dim, _p(rho), 3, _p(cen), 1, 0, _p(want), _capi.QT_HOST_PTR)
    assert rc == 0 and np.all(np.isfinite(want)) and want.max() > 1e-6
    assert np.array_equal(eng.metric_dist(rho, cen, metric), want)
    assert np.array_equal(eng.distance(rho, cen, metric), want)


# ---- 3. Hilbert-Schmidt through `distance` -----------------------------------------------------------------------------
def test_distance_without_a_metric_is_hs_dist(qp):
    import torch

    from quantpy_amd import _capi

    eng = qp.get_engine(2)
    rng = np.random.default_rng(7)
    for dim in (4, 16):  # the engine's own size, and a foreign one
        rho, cen = _density(rng, (5,), dim), _density(rng, (), dim)
        want = eng.hs_dist(rho, cen)
        assert want.min() > 1e-6
        assert np.array_equal(eng.distance(rho, cen), want) and np.array_equal(eng.distance(rho, cen, metric="hs"), want)
    rho, cen = _density(rng, (5,), 4), _density(rng, (), 4)
    raw = np.full(5, np.nan)
    assert eng.lib.qt_hs_dist_batch(eng._h, _p(rho), _p(cen), 5, _p(raw), _capi.QT_HOST_PTR) == 0
    dev = torch.device("cuda", eng.device)
    dist = torch.full((5,), float("nan"), dtype=torch.float64, device=dev)
    eng.distance_dev(torch.from_numpy(rho).to(dev), torch.from_numpy(cen).to(dev), dist)
    eng.sync()
    assert np.array_equal(dist.cpu().numpy(), raw) and np.array_equal(raw, eng.hs_dist(rho, cen))


# ---- 4, 5. state chains ------------------------------------------------------------------------------------------------
def _raw_hits(eng, name, code, counts, centres, x0, thr, seed, burn, n_points, thinning, step):
    from quantpy_amd import _capi

    chains = counts.shape[0]
    hits, acc = np.full(chains, -1, dtype=np.int64), np.full(chains, -1, dtype=np.int64)
    dist = np.full((chains, n_points), np.nan)
    head = () if code is None else (code,)
    rc = getattr(eng.lib, name)(eng._h, *head, _p(counts), chains, _p(centres), _p(x0), _p(thr), seed, 0, burn, n_points,
                                thinning, step, _p(hits), _p(acc), _p(dist), _capi.QT_HOST_PTR)
    assert rc == 0, _capi.last_error()
    return hits, acc, dist


def _chains_match(eng, stem, counts, est, rho, seed, step):
    x0, status = eng.chol_param(est)
    assert not status.any()
    counts, est, x0 = (np.ascontiguousarray(a) for a in (counts, est, x0))
    setting = (2, 3, 2)  # burn_steps, n_points, thinning
    for metric in (None, "trace"):
        thr = np.ascontiguousarray(eng.distance(est, rho, metric))
        name = stem + ("_hits" if metric is None else "_metric_hits")
        want = _raw_hits(eng, name, None if metric is None else eng._METRICS[metric], counts, est, x0, thr, seed, *setting, step)
        got = eng.mhmc_state_hits(counts, est, x0, thr, seed, *setting, step, return_dist=True, metric=metric)
        assert np.all(np.isfinite(want[2])) and want[2].max() > 0
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, a, b)


def test_state_hits_at_four_qubits_is_the_large_entry(qp, oracle):
    n = 4
    counts, rho = large.trial_counts(oracle, n)
    eng = qp.get_engine(n)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * large.SHOTS[n])
    est = eng.lin(counts[:2])
    assert np.linalg.eigvalsh(est).min() > 1e-3  # positive definite centres
    _chains_match(eng, "qt_mhmc_state_large", counts[:2], est, rho, large.DRAW_SEEDS[n], large.STEP)
    assert eng.mhmc_state_large_hits.__func__ is eng.mhmc_state_hits.__func__  # the older name of the same method


def test_state_hits_at_two_qubits_is_the_small_entry(qp, oracle):
    n, chains = 2, 5
    counts, rho = small.trial_counts(oracle, n, chains, 100 * n + chains)
    eng = qp.get_engine(n)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * small.SHOTS)
    _chains_match(eng, "qt_mhmc_state", counts, eng.lin(counts), rho, 2026, 2.0)


# ---- 6. the draws ------------------------------------------------------------------------------------------------------
def test_the_three_draws_entries_give_one_table_at_one_length(qp, oracle):
    seed, chains, steps, c0, s0 = 0xFEDCBA9876543210, 3, 5, (1 << 32) + 3, 2
    two = qp.get_engine(2)  # D = 16
    one = qp.get_engine(1)  # D^2 = 16
    one.set_povm(qp.generate_measurement_matrix("proj-set", 1), np.ones(3) * small.SHOTS)
    one.process_setup(oracle.input_states("proj4", 1))
    state = two.mhmc_draws(seed, chains, steps, first_chain=c0, first_step=s0)
    process = one.mhmc_process_draws(seed, chains, steps, first_chain=c0, first_step=s0)
    by_dim = one.mhmc_draws_dim(16, seed, chains, steps, first_chain=c0, first_step=s0)
    assert state[0].shape == (chains, steps, 16) and np.all(np.isfinite(state[0])) and np.ptp(state[0]) > 1
    for other in (process, by_dim):
        assert np.array_equal(other[0], state[0]) and np.array_equal(other[1], state[1])
