"""GPU: the process chain study in trace distance and infidelity -- qt_mhmc_process_metric_hits,
metrics.get_CL_list_channel_mhmc(dst='trace' | 'if').

The batches, steps, settings and Philox seeds of tests/test_gpu_process_mhmc_coverage.py (process_mhmc_coverage_cases):
n, C = (1, 1), (1, 5), (2, 3); the accepted steps do not depend on the distance, so its acceptance shares hold here.  At
n = 1 the chain's one wavefront measures its 4 x 4 matrix in the lane-group form (four groups holding the same matrix), at
n = 2 the workgroup of 256 threads in the form of qt_metric_dist_dim's dim = 16 kernel.

The fused kernel is compared with the UNFUSED composition: qt_mhmc_process_draws -> qt_mhmc_process -> the real parts of
the kept states -> qt_metric_dist_dim against the chain's centre.  Both sides run the same device functions on the same
inputs, so the design target is equal bits; the bound is the sibling's TOL = 1e-13 absolute.

Centres.  Trace distance: the chain's starting point x0, as in the study.  Infidelity: x0 / 4^n.  A Choi matrix has trace
2^n, so against x0 itself the fidelity is about 4^n, the infidelity negative and returned as 0 (the degenerate case the
study documents); against x0 / 4^n the fidelity is at most 1 and the infidelities are positive and distinct (1e-3 for a
nearly real Choi matrix, up to 0.3 where the real part drops much of a complex one), which exercises the root and both
products.  The conditions that pin the hits -- no unfused distance within TOL of its
threshold, both outcomes of the comparison occur, and (infidelity) the distances are not all clipped to 0 -- are
conditions on the inputs, asserted on the device's own unfused run."""
import numpy as np
import pytest

import process_mhmc_coverage_cases as cases

pytestmark = pytest.mark.gpu

TOL = 1e-13
SETTINGS = cases.SETTINGS
DRAW_SEEDS = {1: 3025, 2: 3026}
METRICS = ["trace", "if"]


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


_BATCHES, _CHAINS, _UNFUSED = {}, {}, {}


def _batch(oracle, n, chains):
    """(povm, input states, counts, true Choi matrices, starting points) of a case, computed once."""
    if (n, chains) not in _BATCHES:
        _BATCHES[n, chains] = cases.trial_batch(oracle, n, chains, cases.batch_seed(n, chains))
    return _BATCHES[n, chains]


def _engine(qp, oracle, n):
    """The cached engine of this size with the tests' POVM and input states (other tests register their own)."""
    povm, ins = _batch(oracle, *next(c for c in cases.CASES if c[0] == n))[:2]
    eng = qp.get_engine(n)
    eng.set_povm(povm, np.ones(3**n) * cases.SHOTS)
    eng.process_setup(ins)
    return eng


def _centres(x0, n, metric):
    return x0 if metric == "trace" else np.ascontiguousarray(x0 / 4**n)


def kept_states(eng, counts, x0, seed, burn, n_points, thinning, step, first_chain=0):
    """The study's chain on entries that predate the fused kernels: (real parts of the kept states (C, n_points, D, D),
    accepted post-burn steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_process_draws(seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_process(counts, x0, deltas, uniforms, step)
    kept = np.ascontiguousarray(chain[:, burn::thinning][:, :n_points].real)
    return kept, acc[:, burn:].sum(axis=1).astype(np.int64)


def unfused(eng, kept, centres, metric):
    return np.stack([eng.metric_dist_dim(kept[c], centres[c], metric) for c in range(kept.shape[0])])


def _reference(qp, oracle, n, chains, setting, metric):
    """(unfused distances, unfused accepted, thresholds) of a case, setting and metric, computed once."""
    key = (n, chains, setting, metric)
    if key not in _UNFUSED:
        povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
        eng = _engine(qp, oracle, n)
        if key[:3] not in _CHAINS:
            _CHAINS[key[:3]] = kept_states(eng, counts, x0, DRAW_SEEDS[n], *SETTINGS[setting], cases.STEPS[n])
        kept, acc = _CHAINS[key[:3]]
        dist = unfused(eng, kept, _centres(x0, n, metric), metric)
        delta = np.array([eng.metric_dist_dim(x0[c], _centres(chois[c], n, metric), metric) for c in range(chains)])
        thr = cases.thresholds(delta, dist)
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _UNFUSED[key] = dist, acc, thr
    return _UNFUSED[key]


# ---- 1. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,chains", cases.CASES)
def test_fused_chain_equals_the_unfused_composition(qp, oracle, n, chains, metric, setting):
    burn, n_points, thinning = SETTINGS[setting]
    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    want_dist, want_acc, thr = _reference(qp, oracle, n, chains, setting, metric)
    eng = _engine(qp, oracle, n)
    args = (DRAW_SEEDS[n], burn, n_points, thinning, cases.STEPS[n])
    hits, acc, dist = eng.mhmc_process_hits(counts, _centres(x0, n, metric), x0, thr, *args, return_dist=True, metric=metric)
    hs_acc = eng.mhmc_process_hits(counts, x0, x0, thr, *args)[1]
    err = np.abs(dist - want_dist).max()
    lo = (thr[:, None] > want_dist + TOL).sum(axis=1)
    hi = (thr[:, None] > want_dist - TOL).sum(axis=1)
    print(f"n={n} C={chains} {metric} {setting}: max |dist - unfused| {err:.2e} (bit-equal: {np.array_equal(dist, want_dist)}), "
          f"distances in [{want_dist.min():.3e}, {want_dist.max():.3e}], {len(np.unique(want_dist))} distinct, "
          f"hits {hits.tolist()} in [{lo.tolist()}, {hi.tolist()}], accepted {acc.tolist()} / unfused {want_acc.tolist()}")
    assert hits.dtype == np.int64 and acc.dtype == np.int64 and dist.shape == (chains, n_points)
    assert np.array_equal(acc, want_acc) and np.array_equal(acc, hs_acc)
    assert err < TOL
    assert not (np.abs(thr[:, None] - want_dist) <= TOL).any()  # the condition on the inputs that pins the hits
    assert np.array_equal(lo, hi) and np.all(lo <= hits) and np.all(hits <= hi)
    assert 0 < hits.sum() < chains * n_points  # both outcomes of the comparison occur
    # not degenerate: every chain has positive, distinct distances; an infidelity lies in [0, 1] -- Re(X) = (X + X^T) / 2
    # and the centre are positive semidefinite with traces 2^n and 2^-n, so the fidelity is at most their product
    assert np.all(want_dist.max(axis=1) > 1e-12) and all(len(np.unique(row)) > 1 for row in want_dist)
    if metric == "if":
        assert want_dist.min() >= 0.0 and want_dist.max() <= 1.0


# ---- 2. position independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,chains,first", [(1, 5, 2), (2, 3, 1)])
def test_chains_do_not_depend_on_their_place_in_the_batch(qp, oracle, n, chains, first, metric):
    """Chains [first, C) computed alone with first_chain = first: the bits of those rows of the whole batch's call."""
    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    cen = _centres(x0, n, metric)
    eng = _engine(qp, oracle, n)
    for setting in sorted(SETTINGS):
        thr = _reference(qp, oracle, n, chains, setting, metric)[2]
        args = (DRAW_SEEDS[n], *SETTINGS[setting], cases.STEPS[n])
        full = eng.mhmc_process_hits(counts, cen, x0, thr, *args, return_dist=True, metric=metric)
        part = eng.mhmc_process_hits(counts[first:], cen[first:], x0[first:], thr[first:], *args, first_chain=first,
                                     return_dist=True, metric=metric)
        for a, b in zip(full, part):
            assert np.array_equal(a[first:], b), (n, setting)
        shifted = eng.mhmc_process_hits(counts[first:], cen[first:], x0[first:], thr[first:], *args, return_dist=True,
                                        metric=metric)
        assert not np.array_equal(shifted[2], part[2])  # (other numbers: first_chain is what keys them)


# ---- 3. pointers and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,chains", [(1, 5), (2, 3)])
def test_pointer_kinds_and_edges(qp, oracle, n, chains, metric):
    import torch

    from quantpy_amd import _capi

    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    cen = _centres(x0, n, metric)
    eng = _engine(qp, oracle, n)
    thr = _reference(qp, oracle, n, chains, "thinned", metric)[2]
    seed, step = DRAW_SEEDS[n], cases.STEPS[n]
    args = (seed, *SETTINGS["thinned"], step)
    hits, acc, dist = eng.mhmc_process_hits(counts, cen, x0, thr, *args, return_dist=True, metric=metric)
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, cen, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_process_hits(*on_dev, *args, return_dist=True, metric=metric)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_process_hits(counts, cen, x0, thr, *args, metric=metric)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN in one centre: NaN distances and no hits for that chain alone, the chain itself (choi_init) untouched
    bad = cen.copy()
    bad[1, 0, -1] = np.nan
    big = np.full(chains, 1e3)  # above every distance: all n_points kept states are hits
    n_hits, n_acc, n_dist = eng.mhmc_process_hits(counts, bad, x0, big, *args, return_dist=True, metric=metric)
    ok = np.arange(chains) != 1
    assert np.isnan(n_dist[1]).all() and n_hits[1] == 0 and np.array_equal(n_acc, acc)
    assert np.array_equal(n_dist[ok], dist[ok]) and np.all(n_hits[ok] == SETTINGS["thinned"][1])
    # C = 0
    empty = eng.mhmc_process_hits(counts[:0], cen[:0], x0[:0], thr[:0], *args, return_dist=True, metric=metric)
    assert [a.shape for a in empty] == [(0,), (0,), (0, SETTINGS["thinned"][1])]
    # what qt_mhmc_process_hits refuses, and an unknown metric
    for wrong in ((seed, 3, 7, 0, step), (seed, -1, 7, 1, step), (seed, 2**31 - 1, 2**31 - 1, 2, step), (seed, 3, -1, 1, step)):
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_process_hits(counts, cen, x0, thr, *wrong, metric=metric)
        assert e.value.code == _capi.QT_ERR_ARG
    with pytest.raises(ValueError):
        eng.mhmc_process_hits(counts, cen, x0, thr, *args, metric="fro")
    h, a = np.zeros(chains, dtype=np.int64), np.zeros(chains, dtype=np.int64)
    for code in (-1, 2):
        rc = eng.lib.qt_mhmc_process_metric_hits(eng._h, code, counts.ctypes.data, chains, cen.ctypes.data, x0.ctypes.data,
                                                 thr.ctypes.data, 1, 0, 3, 7, 2, step, h.ctypes.data, a.ctypes.data, None,
                                                 _capi.QT_HOST_PTR)
        assert rc == _capi.QT_ERR_ARG and "unknown metric" in _capi.last_error()


def test_three_qubits_are_refused_without_a_launch(qp):
    from quantpy_amd import _capi

    eng = qp.get_engine(3)  # (whatever is registered on it: the refusal comes first)
    one = np.zeros(1, dtype=np.int64)
    code = eng.lib.qt_mhmc_process_metric_hits(eng._h, _capi.QT_METRIC_TRACE, one.ctypes.data, 1, one.ctypes.data,
                                               one.ctypes.data, one.ctypes.data, 1, 0, 0, 1, 1, 0.1, one.ctypes.data,
                                               one.ctypes.data, None, _capi.QT_HOST_PTR)
    assert code == _capi.QT_ERR_UNSUPPORTED and "n_qubits 1..2" in _capi.last_error()


def test_entry_needs_the_povm_and_the_process_setup(qp):
    """A fresh handle: QT_ERR_STATE, as qt_mhmc_process_hits gives it, and nothing is launched."""
    from quantpy_amd import _capi

    eng = qp.engine.Engine(1)
    one = np.zeros(1, dtype=np.int64)

    def call():
        return eng.lib.qt_mhmc_process_metric_hits(eng._h, _capi.QT_METRIC_INFIDELITY, one.ctypes.data, 1, one.ctypes.data,
                                                   one.ctypes.data, one.ctypes.data, 1, 0, 0, 1, 1, 0.1, one.ctypes.data,
                                                   one.ctypes.data, None, _capi.QT_HOST_PTR)

    try:
        assert call() == _capi.QT_ERR_STATE and "qt_set_povm" in _capi.last_error()
        eng.set_povm(qp.generate_measurement_matrix("proj-set", 1), np.ones(3) * 1000)
        assert call() == _capi.QT_ERR_STATE and "qt_process_setup" in _capi.last_error()
    finally:
        eng.close()


# ---- 4. the public function ------------------------------------------------------------------------------------------
def _study_kw(n_iter, n_points, burn, step, seed):
    return dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, step=step, n_measurements=cases.SHOTS, sampler="numpy",
                seed=seed)


def test_study_in_trace_distance_reproduces_its_hits_through_the_unfused_path(qp):
    from quantpy_amd import metrics

    n, n_iter, n_points, burn = 1, 3, 20, 3
    channel = qp.channel.depolarizing(0.2, n)
    step = cases.STEPS[n]
    kw = _study_kw(n_iter, n_points, burn, step, 61)
    np.random.seed(401)
    out = metrics.get_CL_list_channel_mhmc(channel, return_details=True, dst="trace", **kw)
    assert out["seed"] == 62 and out["counts"].shape[0] == n_iter
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    tmg.experiment_batch(cases.SHOTS, "proj-set", repeats=1)  # (registers the POVM and the shots on the tomograph)
    eng = tmg._engine()
    kept, acc = kept_states(eng, out["counts"], out["estimates"], out["seed"], burn, n_points, 1, step)
    dist = unfused(eng, kept, out["estimates"], "trace")
    assert not (np.abs(out["delta"][:, None] - dist) <= TOL).any()  # the condition that pins the hits
    hits = (out["delta"][:, None] > dist).sum(axis=1)
    print(f"study: hits {out['hits'].tolist()} / unfused {hits.tolist()}, accepted {acc.tolist()}")
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["acceptance_rate"], acc / n_points)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    assert np.array_equal(out["delta"], eng.metric_dist_dim(out["estimates"], channel.choi.matrix, "trace"))
    np.random.seed(401)
    hs = metrics.get_CL_list_channel_mhmc(channel, return_details=True, dst="hs", **kw)
    np.random.seed(401)
    plain = metrics.get_CL_list_channel_mhmc(channel, return_details=True, **kw)
    for k in plain:
        assert np.array_equal(plain[k], hs[k]), k
    assert np.array_equal(plain["acceptance_rate"], out["acceptance_rate"])  # the same chains, whatever the distance


def test_study_in_infidelity_is_degenerate_as_documented(qp):
    """Choi matrices have trace 2^n: if_dst of two of them is 1 - (about 2^n)^2 < 1e-15 and is returned as 0, as
    geometry.py:52-54 returns it.  Every delta, every hit count and every level is 0."""
    from quantpy_amd import metrics

    out = metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.2, 1), return_details=True, dst="if",
                                           **_study_kw(3, 20, 3, cases.STEPS[1], 61))
    assert not out["delta"].any() and not out["hits"].any() and not out["levels"].any()
    assert out["acceptance_rate"].max() > 0  # (the chains ran)


def test_study_refuses_a_three_qubit_channel(qp):
    from quantpy_amd import metrics

    with pytest.raises(NotImplementedError, match="one and two qubits"):
        metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1, dst="trace")
