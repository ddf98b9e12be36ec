"""GPU: the state chain study in trace distance and infidelity -- qt_mhmc_state_metric_hits,
metrics.get_CL_list_state_mhmc(dst='trace' | 'if').

Batches of tests/mhmc_coverage_cases.py as tests/test_gpu_mhmc_coverage.py runs them, n, C = (1, 5), (2, 5), (3, 2): at
n = 1 five chains share a wavefront (16 per wavefront) and at n = 2 they cross a wavefront boundary (4 per wavefront), each
with its own matrix and therefore its own number of Jacobi sweeps; both step settings, (burn_steps, n_points, thinning) =
(3, 7, 2) and (0, 40, 1); STEP and the Philox seeds of the sibling (the accepted steps do not depend on the distance, so
its acceptance shares hold here).

The fused kernel is compared with the UNFUSED composition: qt_mhmc_draws -> qt_mhmc_state -> qt_chol_unparam ->
qt_metric_dist_group_batch on the kept states.  Both sides run the same device functions on the same inputs, so the
design target is equal bits; the bound is the sibling's TOL = 1e-13 absolute.  The condition that pins the hits -- no
unfused distance within TOL of its threshold, both outcomes of the comparison occur -- is a condition on the inputs,
asserted on the device's own unfused run."""
import numpy as np
import pytest

import mhmc_coverage_cases as cases

pytestmark = pytest.mark.gpu

STEP = 2.0
TOL = 1e-13
SETTINGS = {"thinned": (3, 7, 2), "plain": (0, 40, 1)}  # burn_steps, n_points, thinning
CASES = [(1, 5), (2, 5), (3, 2)]
METRICS = ["trace", "if"]
DRAW_SEEDS = {1: 2025, 2: 2026, 3: 7581}


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _engine(qp, n):
    eng = qp.get_engine(n)  # (the cached engine of this size: other tests register their own POVM)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * cases.SHOTS)
    return eng


_BATCHES, _CHAINS, _UNFUSED = {}, {}, {}


def _batch(qp, oracle, n, chains):
    """(counts, estimates, true state, x0) of a case, computed once."""
    if (n, chains) not in _BATCHES:
        counts, rho = cases.trial_counts(oracle, n, chains, 100 * n + chains)
        eng = _engine(qp, n)
        est = eng.lin(counts)
        x0, status = eng.chol_param(est)
        assert not status.any()
        _BATCHES[n, chains] = counts, est, rho, x0
    return _BATCHES[n, chains]


def kept_states(eng, counts, x0, seed, burn, n_points, thinning, step, first_chain=0):
    """The study's chain on entries that predate the fused kernels: (kept states (C, n_points, d, d), accepted post-burn
    steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_draws(seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, step)
    kept = chain[:, burn::thinning][:, :n_points]
    mats = eng.chol_unparam(kept.reshape(-1, eng.D)).reshape(chains, n_points, eng.d, eng.d)
    return mats, acc[:, burn:].sum(axis=1).astype(np.int64)


def unfused(eng, mats, centres, metric):
    return np.stack([eng.metric_dist(mats[c], centres[c], metric) for c in range(mats.shape[0])])


def _median_off_samples(dist):
    """A threshold in the middle of one chain's distances and on none of them."""
    s = np.unique(dist)
    return 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) > 1 else 1.5 * s[0] + 1e-3


def _reference(qp, oracle, n, chains, setting, metric):
    """(unfused distances, unfused accepted, thresholds), computed once: the thresholds are the trial's own delta in
    `metric` for the odd chains and the nudged median of the chain's unfused distances for the even ones."""
    key = (n, chains, setting, metric)
    if key not in _UNFUSED:
        counts, est, rho, x0 = _batch(qp, oracle, n, chains)
        eng = _engine(qp, n)
        if key[:3] not in _CHAINS:
            _CHAINS[key[:3]] = kept_states(eng, counts, x0, DRAW_SEEDS[n], *SETTINGS[setting], STEP)
        mats, acc = _CHAINS[key[:3]]
        dist = unfused(eng, mats, est, metric)
        delta = eng.metric_dist(est, rho, metric)
        thr = np.array([delta[c] if c % 2 else _median_off_samples(dist[c]) for c in range(chains)])
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _UNFUSED[key] = dist, acc, thr
    return _UNFUSED[key]


# ---- 1. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,chains", CASES)
def test_fused_chain_equals_the_unfused_composition(qp, oracle, n, chains, metric, setting):
    burn, n_points, thinning = SETTINGS[setting]
    counts, est, rho, x0 = _batch(qp, oracle, n, chains)
    want_dist, want_acc, thr = _reference(qp, oracle, n, chains, setting, metric)
    eng = _engine(qp, n)
    args = (DRAW_SEEDS[n], burn, n_points, thinning, STEP)
    hits, acc, dist = eng.mhmc_state_hits(counts, est, x0, thr, *args, return_dist=True, metric=metric)
    hs_acc = eng.mhmc_state_hits(counts, est, x0, thr, *args)[1]
    err = np.abs(dist - want_dist).max()
    lo = (thr[:, None] > want_dist + TOL).sum(axis=1)
    hi = (thr[:, None] > want_dist - TOL).sum(axis=1)
    print(f"n={n} C={chains} {metric} {setting}: max |dist - unfused| {err:.2e} (bit-equal: {np.array_equal(dist, want_dist)}), "
          f"distances in [{want_dist.min():.3e}, {want_dist.max():.3e}], hits {hits.tolist()} in [{lo.tolist()}, {hi.tolist()}], "
          f"accepted {acc.tolist()} / unfused {want_acc.tolist()}")
    assert hits.dtype == np.int64 and acc.dtype == np.int64 and dist.shape == (chains, n_points)
    assert np.array_equal(acc, want_acc) and np.array_equal(acc, hs_acc)
    assert err < TOL
    assert not (np.abs(thr[:, None] - want_dist) <= TOL).any()  # the condition on the inputs that pins the hits
    assert np.array_equal(lo, hi) and np.all(lo <= hits) and np.all(hits <= hi)
    assert 0 < hits.sum() < chains * n_points  # both outcomes of the comparison occur
    assert np.ptp(want_dist) > 1e-3  # (the distances are not degenerate)


# ---- 2. position independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2])
def test_chains_do_not_depend_on_their_place_in_the_batch(qp, oracle, n, metric):
    """Chains [2, 5) computed alone with first_chain = 2: the bits of rows 2..4 of the C = 5 call (n = 1, 2: the chains
    then sit in other lane groups, with other wavefront neighbours)."""
    counts, est, rho, x0 = _batch(qp, oracle, n, 5)
    eng = _engine(qp, n)
    for setting in sorted(SETTINGS):
        thr = _reference(qp, oracle, n, 5, setting, metric)[2]
        args = (DRAW_SEEDS[n], *SETTINGS[setting], STEP)
        full = eng.mhmc_state_hits(counts, est, x0, thr, *args, return_dist=True, metric=metric)
        part = eng.mhmc_state_hits(counts[2:], est[2:], x0[2:], thr[2:], *args, first_chain=2, return_dist=True, metric=metric)
        for a, b in zip(full, part):
            assert np.array_equal(a[2:], b), (n, setting)
        shifted = eng.mhmc_state_hits(counts[2:], est[2:], x0[2:], thr[2:], *args, return_dist=True, metric=metric)
        assert not np.array_equal(shifted[2], part[2])  # (other numbers: first_chain is what keys them)


# ---- 3. pointers and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,chains", CASES)
def test_pointer_kinds_and_edges(qp, oracle, n, chains, metric):
    import torch

    from quantpy_amd import _capi

    counts, est, rho, x0 = _batch(qp, oracle, n, chains)
    eng = _engine(qp, n)
    thr = _reference(qp, oracle, n, chains, "thinned", metric)[2]
    args = (DRAW_SEEDS[n], *SETTINGS["thinned"], STEP)
    hits, acc, dist = eng.mhmc_state_hits(counts, est, x0, thr, *args, return_dist=True, metric=metric)
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, est, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_state_hits(*on_dev, *args, return_dist=True, metric=metric)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_state_hits(counts, est, x0, thr, *args, metric=metric)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN in one centre: NaN distances and no hits for that chain alone, the chain itself (x_init) untouched
    bad = est.copy()
    bad[1, 0, -1] = np.nan
    big = np.full(chains, 10.0)  # above every distance: all n_points kept states are hits
    n_hits, n_acc, n_dist = eng.mhmc_state_hits(counts, bad, x0, big, *args, return_dist=True, metric=metric)
    ok = np.arange(chains) != 1
    assert np.isnan(n_dist[1]).all() and n_hits[1] == 0 and np.array_equal(n_acc, acc)
    assert np.array_equal(n_dist[ok], dist[ok]) and np.all(n_hits[ok] == SETTINGS["thinned"][1])
    # C = 0
    empty = eng.mhmc_state_hits(counts[:0], est[:0], x0[:0], thr[:0], *args, return_dist=True, metric=metric)
    assert [a.shape for a in empty] == [(0,), (0,), (0, SETTINGS["thinned"][1])]
    # what qt_mhmc_state_hits refuses, and an unknown metric
    for wrong in ((DRAW_SEEDS[n], 3, 7, 0, STEP), (DRAW_SEEDS[n], -1, 7, 1, STEP), (DRAW_SEEDS[n], 2**31 - 1, 2**31 - 1, 2, STEP)):
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_state_hits(counts, est, x0, thr, *wrong, metric=metric)
        assert e.value.code == _capi.QT_ERR_ARG
    with pytest.raises(ValueError):
        eng.mhmc_state_hits(counts, est, x0, thr, *args, metric="fro")
    h, a = np.zeros(chains, dtype=np.int64), np.zeros(chains, dtype=np.int64)
    for code in (-1, 2):
        rc = eng.lib.qt_mhmc_state_metric_hits(eng._h, code, counts.ctypes.data, chains, est.ctypes.data, x0.ctypes.data,
                                               thr.ctypes.data, 1, 0, 3, 7, 2, STEP, h.ctypes.data, a.ctypes.data, None,
                                               _capi.QT_HOST_PTR)
        assert rc == _capi.QT_ERR_ARG and "unknown metric" in _capi.last_error()


def test_four_qubits_are_refused_without_a_launch(qp):
    from quantpy_amd import _capi

    eng = qp.get_engine(4)  # (no POVM registered: the refusal comes first)
    one = np.zeros(1, dtype=np.int64)
    code = eng.lib.qt_mhmc_state_metric_hits(eng._h, _capi.QT_METRIC_TRACE, one.ctypes.data, 1, one.ctypes.data,
                                             one.ctypes.data, one.ctypes.data, 1, 0, 0, 1, 1, 0.1, one.ctypes.data,
                                             one.ctypes.data, None, _capi.QT_HOST_PTR)
    assert code == _capi.QT_ERR_UNSUPPORTED and "n_qubits 1..3" in _capi.last_error()


# ---- 4. the public function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [1, 2])
def test_study_reproduces_its_hits_through_the_unfused_path(qp, n, metric):
    from quantpy_amd import geometry, metrics

    state = qp.Qobj(cases.mixed_ghz(n))
    n_iter, n_points, burn = 4, 30, 3
    kw = dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, step=STEP, sampler="numpy", seed=40 + n)
    np.random.seed(300 + n)
    out = metrics.get_CL_list_state_mhmc(state, return_details=True, dst=metric, **kw)
    assert out["seed"] == 41 + n and out["counts"].shape[0] == n_iter
    tmg = qp.StateTomograph(state)
    tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", n)
    tmg.n_measurements = np.ones(tmg.povm_matrix.shape[0]) * 1000
    eng = tmg._engine()
    x0, status = eng.chol_param(out["estimates"])
    assert not status.any()
    mats, acc = kept_states(eng, out["counts"], x0, out["seed"], burn, n_points, 1, STEP)
    dist = unfused(eng, mats, out["estimates"], metric)
    assert not (np.abs(out["delta"][:, None] - dist) <= TOL).any()  # the condition that pins the hits
    hits = (out["delta"][:, None] > dist).sum(axis=1)
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["acceptance_rate"], acc / n_points)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    assert np.array_equal(out["delta"], eng.metric_dist(out["estimates"], state.matrix, metric))
    # the functions of quantpy_amd.geometry name the same distances
    np.random.seed(300 + n)
    by_fn = metrics.get_CL_list_state_mhmc(state, dst={"trace": geometry.trace_dst, "if": geometry.if_dst}[metric], **kw)
    assert np.array_equal(by_fn, np.sort(out["levels"]))


@pytest.mark.parametrize("n", [1, 2])
def test_study_in_hs_is_the_call_without_dst(qp, n):
    from quantpy_amd import metrics

    state = qp.Qobj(cases.mixed_ghz(n))
    kw = dict(n_iter=4, n_points=30, burn_steps=3, step=STEP, sampler="device", seed=50 + n, return_details=True)
    plain, hs = metrics.get_CL_list_state_mhmc(state, **kw), metrics.get_CL_list_state_mhmc(state, dst="hs", **kw)
    assert sorted(plain) == sorted(hs)
    for k in plain:
        assert np.array_equal(plain[k], hs[k]), k
