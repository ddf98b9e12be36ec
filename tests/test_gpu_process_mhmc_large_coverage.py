"""GPU: the chain coverage study of three-qubit channels -- qt_mhmc_process_large_hits, qt_mhmc_process_large_metric_hits,
metrics.get_CL_list_channel_mhmc_large.

Batches (process_mhmc_large_coverage_cases): C = 1 and C = 3 chains on three-qubit tomographies of three channels -- the
two of test_gpu_batch_positions.n3_processes and a depolarized Toffoli gate -- 10 000 shots per setting of 'proj-set' on the
'proj4' input states; two step settings, (burn_steps, n_points, thinning) = (2, 5, 2) and (0, 12, 1): at most 12 steps of
at most 3 chains.  Every chain starts from `eng.lifp(counts, cptp=True)`, which is also its centre.  STEP = 1e-5.

The fused launch family is compared with the UNFUSED composition of entries that predate it: the draws written out by
qt_mhmc_draws_dim(dim = 4096) fed to qt_mhmc_process, the real parts of the kept states through qt_hs_dist_dim /
qt_metric_dist_mat against the chain's own centre.  `accepted` is equal exactly (the proposal's element, the NLL's sum and
the accept rule are one device function each in both families).  Tolerance of a Hilbert-Schmidt distance, 1e-12 absolute:
only the order of the distance's own 4096-term sum differs; for a Hermitian centre the terms Delta_ij Delta_ji are
non-negative, so any order is within 4096 * 2^-52 = 9.1e-13 relative on the sum and half of that on the root, on
distances below 1.  Trace distances and infidelities are equal exactly: the same kernel measures the same matrix.  With
'if' every distance of two Choi matrices of trace 8 is 0, as at n <= 2: hits = 0, and the chains ran.

The unfused reference itself runs k_mhmc64_propose / k_mhmc64_decide, which now call the same shared device functions as
the fused kernels: what keeps it an independent reference is that the tests which pin qt_mhmc_process at n = 3 to the
reference implementation pass unchanged (test_gpu_process3.test_n3_mhmc_process_interval_matches_the_reference on the
golden mhmc3, test_gpu_batch_positions.test_n3_process_chains_of_a_batch_equal_the_chains_alone).

The oracle's dense n = 3 operator is not affordable, so the Philox seed of the draws was chosen by running the unfused
composition on the GPU, asking of every case and setting, in 'hs' and 'trace': 0.05 < acceptance share < 0.95,
0 < hits.sum() < C n_points, no distance within 1e-12 of its threshold.  3027, the first seed tried, passed.  That run,
settings (2, 5, 2) / (0, 12, 1), the same in 'hs' and 'trace':
    C = 1: acceptance share 0.600 / 0.667, accepted [6] / [8], hits [2] / [7]
    C = 3: 0.600 / 0.639, accepted [6, 6, 6] / [8, 8, 7], hits [2, 5, 2] / [7, 12, 5]
    Hilbert-Schmidt distances 0.074 .. 0.117, trace distances 0.246 .. 0.500
(a change of the draws' definition or of the batches needs a new search).  The test asserts the conditions on the device's
own unfused run."""
import numpy as np
import pytest

import process_mhmc_large_coverage_cases as cases

pytestmark = pytest.mark.gpu

TOL = 1e-12
SETTINGS = cases.SETTINGS
STEP = cases.STEP
DRAW_SEED = 3027  # Philox seed of the chains (module docstring)
METRICS = [None, "trace", "if"]  # None: Hilbert-Schmidt


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


_CACHE = {}


def _batch(qp):
    """(engine, counts (3, ...), true Choi matrices, starting points = centres), computed once."""
    if "batch" not in _CACHE:
        tmg, counts, truths = cases.tomographs(qp)
        eng = tmg._engine()
        x0 = np.ascontiguousarray(eng.lifp(counts, cptp=True))
        for a in (counts, truths, x0):
            a.setflags(write=False)
        _CACHE["batch"] = tmg, counts, truths, x0
    tmg, counts, truths, x0 = _CACHE["batch"]
    return tmg._engine(), counts, truths, x0  # (the tomograph's engine: POVM, shots and input states registered)


def unfused(eng, counts, centres, seed, burn, n_points, thinning, step, first_chain=0, metric=None):
    """The study's chain on entries that predate the fused family: (kept distances (C, n_points), accepted post-burn
    steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_draws_dim(cases.DIM, seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_process(counts, centres, deltas, uniforms, step)
    kept = np.ascontiguousarray(chain[:, burn::thinning][:, :n_points].real)
    dist = np.stack([eng.distance(kept[c], centres[c], metric) for c in range(chains)])
    return dist, acc[:, burn:].sum(axis=1).astype(np.int64)


def _reference(qp, chains, setting, metric):
    """(unfused distances, unfused accepted, thresholds) of a case, setting and metric, computed once."""
    key = (chains, setting, metric)
    if key not in _CACHE:
        eng, counts, truths, x0 = _batch(qp)
        counts, truths, x0 = counts[:chains], truths[:chains], x0[:chains]
        dist, acc = unfused(eng, counts, x0, DRAW_SEED, *SETTINGS[setting], STEP, metric=metric)
        delta = np.array([eng.distance(x0[c], truths[c], metric) for c in range(chains)])
        thr = delta if metric == "if" else cases.thresholds(delta, dist)
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _CACHE[key] = dist, acc, thr
    return _CACHE[key]


# ---- 1. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("chains", cases.CASES)
def test_fused_chain_equals_the_unfused_composition(qp, chains, setting, metric):
    burn, n_points, thinning = SETTINGS[setting]
    eng, counts, truths, x0 = _batch(qp)
    counts, x0 = counts[:chains], x0[:chains]
    want_dist, want_acc, thr = _reference(qp, chains, setting, metric)
    hits, acc, dist = eng.mhmc_process_hits(counts, x0, x0, thr, DRAW_SEED, burn, n_points, thinning, STEP, return_dist=True,
                                            metric=metric)
    share = want_acc.sum() / (chains * n_points * thinning)
    err = np.abs(dist - want_dist).max()
    lo = (thr[:, None] > want_dist + TOL).sum(axis=1)
    hi = (thr[:, None] > want_dist - TOL).sum(axis=1)
    print(f"C={chains} {setting} {metric or 'hs'}: acceptance share {share:.3f}, max |dist - unfused| {err:.2e}, hits "
          f"{hits.tolist()} in [{lo.tolist()}, {hi.tolist()}], accepted {acc.tolist()} / unfused {want_acc.tolist()}, "
          f"distances {want_dist.min():.3e} .. {want_dist.max():.3e}")
    assert hits.dtype == np.int64 and acc.dtype == np.int64 and dist.shape == (chains, n_points)
    assert np.array_equal(acc, want_acc)
    assert 0.05 < share < 0.95  # both branches of the step run
    if metric == "if":  # degenerate, as documented: every distance and every threshold is 0
        assert not want_dist.any() and not thr.any() and not dist.any() and not hits.any()
        return
    if metric is None:
        assert err < TOL and want_dist.max() < 1.0
    else:
        assert np.array_equal(dist, want_dist)
    assert not (np.abs(thr[:, None] - want_dist) <= TOL).any()  # a condition on the inputs: the hits are pinned
    assert np.array_equal(lo, hi) and np.all(lo <= hits) and np.all(hits <= hi)
    assert 0 < hits.sum() < chains * n_points  # both outcomes of the comparison occur


def test_metric_entry_accepts_the_steps_of_the_hs_entry(qp):
    eng, counts, truths, x0 = _batch(qp)
    args = (DRAW_SEED, *SETTINGS["thinned"], STEP)
    thr = _reference(qp, 3, "thinned", None)[2]
    acc = eng.mhmc_process_hits(counts, x0, x0, thr, *args)[1]
    for metric in ("trace", "if"):
        assert np.array_equal(eng.mhmc_process_hits(counts, x0, x0, thr, *args, metric=metric)[1], acc)
    assert eng.mhmc_process_large_hits.__func__ is eng.mhmc_process_hits.__func__  # (the alias)


# ---- 2. position independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [None, "trace"])
def test_chains_do_not_depend_on_their_place_in_the_batch(qp, metric):
    """Chains [1, 3) computed alone with first_chain = 1: the bits of those rows of the whole batch's call."""
    eng, counts, truths, x0 = _batch(qp)
    first = 1
    for setting in sorted(SETTINGS):
        thr = _reference(qp, 3, setting, metric)[2]
        args = (DRAW_SEED, *SETTINGS[setting], STEP)
        full = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True, metric=metric)
        part = eng.mhmc_process_hits(counts[first:], x0[first:], x0[first:], thr[first:], *args, first_chain=first,
                                     return_dist=True, metric=metric)
        for a, b in zip(full, part):
            assert np.array_equal(a[first:], b), (setting, metric)
        shifted = eng.mhmc_process_hits(counts[first:], x0[first:], x0[first:], thr[first:], *args, return_dist=True,
                                        metric=metric)
        assert not np.array_equal(shifted[2], part[2])  # (other numbers: first_chain is what keys them)


# ---- 3. the slice seam -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [None, "trace", "if"])
def test_slices_are_invisible_in_the_results(qp, metric):
    """C = 3 in slices of 2 (a full slice and a remainder of one chain) against the default's one slice, bit for bit."""
    from quantpy_amd import _capi

    eng, counts, truths, x0 = _batch(qp)
    thr = _reference(qp, 3, "thinned", metric)[2]
    args = (DRAW_SEED, *SETTINGS["thinned"], STEP)
    whole = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True, metric=metric)
    eng.set_option(_capi.QT_OPT_MHMC_PROCESS_SLICE, 2)
    try:
        sliced = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True, metric=metric)
    finally:
        eng.set_option(_capi.QT_OPT_MHMC_PROCESS_SLICE, 0)
    for a, b in zip(whole, sliced):
        assert np.array_equal(a, b), metric
    with pytest.raises(qp.engine.EngineError) as e:
        eng.set_option(_capi.QT_OPT_MHMC_PROCESS_SLICE, -1)
    assert e.value.code == _capi.QT_ERR_ARG


# ---- 4. pointers and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [None, "trace"])
def test_pointer_kinds_and_edges(qp, metric):
    import torch

    chains = 3
    eng, counts, truths, x0 = _batch(qp)
    thr = _reference(qp, chains, "thinned", metric)[2]
    seed, step = DRAW_SEED, STEP
    args = (seed, *SETTINGS["thinned"], step)
    hits, acc, dist = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True, metric=metric)
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, x0, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_process_hits(*on_dev, *args, return_dist=True, metric=metric)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_process_hits(counts, x0, x0, thr, *args, metric=metric)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN threshold never counts
    nan_hits, nan_acc = eng.mhmc_process_hits(counts, x0, x0, np.full(chains, np.nan), *args, metric=metric)
    assert not nan_hits.any() and np.array_equal(nan_acc, acc)
    # C = 0
    empty = eng.mhmc_process_hits(counts[:0], x0[:0], x0[:0], thr[:0], *args, return_dist=True, metric=metric)
    assert [a.shape for a in empty] == [(0,), (0,), (0, SETTINGS["thinned"][1])]
    # argument errors of the entry: thinning < 1, burn_steps < 0, burn_steps + n_points * thinning >= 2^32 - 1
    for bad in ((seed, 3, 7, 0, step), (seed, -1, 7, 1, step), (seed, 2**31 - 1, 2**31 - 1, 2, step)):
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_process_hits(counts, x0, x0, thr, *bad, metric=metric)
        assert e.value.code == qp._capi.QT_ERR_ARG
    with pytest.raises(qp.engine.EngineError) as e:
        eng.mhmc_process_hits(counts, x0, x0, thr, seed, 3, -1, 1, step, metric=metric)  # n_points < 0
    assert e.value.code == qp._capi.QT_ERR_ARG
    if metric is not None:
        code = eng.lib.qt_mhmc_process_large_metric_hits(eng._h, 7, None, 0, None, None, None, 1, 0, 0, 1, 1, 0.1, None, None,
                                                         None, qp._capi.QT_HOST_PTR)
        assert code == qp._capi.QT_ERR_ARG and "unknown metric" in qp._capi.last_error()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def _both_entries(eng):
    from quantpy_amd import _capi

    one = np.zeros(1, dtype=np.int64)
    p = one.ctypes.data
    yield "qt_mhmc_process_hits", eng.lib.qt_mhmc_process_large_hits(eng._h, p, 1, p, p, p, 1, 0, 0, 1, 1, 0.1, p, p, None,
                                                                     _capi.QT_HOST_PTR)
    yield "qt_mhmc_process_metric_hits", eng.lib.qt_mhmc_process_large_metric_hits(eng._h, _capi.QT_METRIC_TRACE, p, 1, p, p, p,
                                                                                   1, 0, 0, 1, 1, 0.1, p, p, None,
                                                                                   _capi.QT_HOST_PTR)


@pytest.mark.parametrize("n", [1, 2])
def test_smaller_handles_are_refused_without_a_launch(qp, n):
    from quantpy_amd import _capi

    eng = qp.get_engine(n)  # (whatever is registered on it: the refusal comes first)
    for sibling, code in _both_entries(eng):
        assert code == _capi.QT_ERR_UNSUPPORTED and sibling in _capi.last_error()


def test_entries_need_the_povm_and_the_process_setup(qp):
    """A fresh n = 3 handle: QT_ERR_STATE in the siblings' order, and nothing is launched."""
    from quantpy_amd import _capi

    eng = qp.engine.Engine(3)
    try:
        for _, code in _both_entries(eng):
            assert code == _capi.QT_ERR_STATE and "qt_set_povm" in _capi.last_error()
        eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * 1000)
        for _, code in _both_entries(eng):
            assert code == _capi.QT_ERR_STATE and "qt_process_setup" in _capi.last_error()
    finally:
        eng.close()


# ---- 6. the public function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", ["hs", "trace"])
def test_study_reproduces_its_hits_through_the_unfused_path(qp, dst):
    from quantpy_amd import metrics

    channel = qp.channel.depolarizing(0.2, 3)
    n_iter, n_points, burn = 3, 5, 2
    metric = None if dst == "hs" else dst
    kw = dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, step=STEP, n_measurements=cases.SHOTS, sampler="numpy",
              seed=63, dst=dst)
    np.random.seed(403)
    out = metrics.get_CL_list_channel_mhmc_large(channel, return_details=True, **kw)
    assert out["seed"] == 64 and out["counts"].shape[0] == n_iter
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    tmg.experiment_batch(cases.SHOTS, "proj-set", repeats=1)  # (registers the POVM and the shots on the tomograph)
    eng = tmg._engine()
    dist, acc = unfused(eng, out["counts"], out["estimates"], out["seed"], burn, n_points, 1, STEP, metric=metric)
    assert not (np.abs(out["delta"][:, None] - dist) <= TOL).any()  # the condition that pins the hits
    hits = (out["delta"][:, None] > dist).sum(axis=1)
    print(f"n=3 study {dst}: hits {out['hits'].tolist()} / unfused {hits.tolist()}, accepted {acc.tolist()}")
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["acceptance_rate"], acc / n_points)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    assert np.array_equal(out["delta"], eng.distance(out["estimates"], channel.choi.matrix, metric))


def test_study_at_one_qubit_is_the_smaller_study(qp):
    from quantpy_amd import metrics

    channel = qp.channel.depolarizing(0.2, 1)
    kw = dict(n_iter=4, n_points=7, burn_steps=3, step=0.006, n_measurements=2000, sampler="numpy", seed=61)
    np.random.seed(401)
    small = metrics.get_CL_list_channel_mhmc(channel, **kw)
    np.random.seed(401)
    assert np.array_equal(metrics.get_CL_list_channel_mhmc_large(channel, **kw), small)
