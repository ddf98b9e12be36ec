"""GPU: the process chain coverage study -- qt_mhmc_process_draws, qt_mhmc_process_hits, metrics.get_CL_list_channel_mhmc.

Batches: n = 1 with C = 1 and C = 5 chains, n = 2 with C = 3 (one workgroup per chain: 64 threads of which 16 hold an
element at n = 1, 256 at n = 2); two step settings, (burn_steps, n_points, thinning) = (3, 7, 2) and (0, 40, 1).  Every
chain has its own channel (depolarizing, amplitude damping / a unitary, Kraus rank 2, with their own parameters) and its
own counts, 2000 shots per setting of 'proj-set' on the 'proj4' input states, and starts from the CPTP-projected 'lifp'
estimate of those counts, which is also its centre.

The fused kernel is compared with the UNFUSED composition of entries that predate it: the draws dumped by
qt_mhmc_process_draws fed to qt_mhmc_process, the real parts of the kept states through qt_hs_dist_dim against the
chain's own centre.  `accepted` is equal exactly (both kernels run ONE device step function on the same numbers);
tolerance of a distance, 1e-13 absolute: only the distance's own sum of <= 256 terms can differ, <= 256 eps relative, on
distances below 1.

The steps, 0.006 (n = 1) and 0.0006 (n = 2), are those at which test_gpu_batch_positions.py gets acceptance 0.2 - 0.8 with
2000 shots (the process likelihood uses the raw counts and is sharp).  The Philox seeds of the draws were chosen by
running the unfused study on the CPU (process_mhmc_coverage_cases.cpu_study: the host instantiation of the draws, the
chain restated in NumPy on the oracle's CPTP projection), asking of every case and setting 0.05 < acceptance share < 0.95,
0 < hits.sum() < C n_points and no distance within 1e-10 of its threshold: 3025 (n = 1) and 3026 (n = 2), the first seeds
tried, passed.  That run, settings (3, 7, 2) / (0, 40, 1):
    n = 1, C = 1: acceptance share 0.143 / 0.325, hits [3] / [25]
    n = 1, C = 5: 0.186 / 0.285, hits [3, 2, 2, 7, 5] / [25, 7, 15, 40, 16]
    n = 2, C = 3: 0.429 / 0.417, hits [2, 0, 4] / [19, 0, 20]
(a change of the draws' definition or of the batches needs a new search).  The test asserts the conditions on the
device's own unfused run."""
import numpy as np
import pytest

import process_mhmc_coverage_cases as cases

pytestmark = pytest.mark.gpu

TOL = 1e-13
SETTINGS = cases.SETTINGS
DRAW_SEEDS = {1: 3025, 2: 3026}  # Philox seeds of the chains (module docstring)


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return cases.build_host_draws(tmp_path_factory.mktemp("process_mhmc_draws"))


_BATCHES, _UNFUSED = {}, {}


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


def unfused(eng, counts, centres, seed, burn, n_points, thinning, step, first_chain=0):
    """The study's chain on entries that predate the fused kernel: (kept distances (C, n_points), accepted post-burn
    steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_process_draws(seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_process(counts, centres, deltas, uniforms, step)
    kept = np.ascontiguousarray(chain[:, burn::thinning][:, :n_points].real)
    dist = np.stack([eng.hs_dist(kept[c], centres[c]) for c in range(chains)])
    return dist, acc[:, burn:].sum(axis=1).astype(np.int64)


def _reference(qp, oracle, n, chains, setting):
    """(unfused distances, unfused accepted, thresholds) of a case and setting, computed once."""
    key = (n, chains, setting)
    if key not in _UNFUSED:
        povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
        eng = _engine(qp, oracle, n)
        dist, acc = unfused(eng, counts, x0, DRAW_SEEDS[n], *SETTINGS[setting], cases.STEPS[n])
        delta = np.array([eng.hs_dist(x0[c], chois[c]) for c in range(chains)])
        thr = cases.thresholds(delta, dist)
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _UNFUSED[key] = dist, acc, thr
    return _UNFUSED[key]


# ---- 1. the draws against their definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_draws_are_the_host_functions(qp, oracle, host_draws, n):
    """Uniforms bit for bit, increments to 1e-13 absolute (|r| <= 8.6, the argument 2 pi u2 rounds to <= 6.3 eps, the
    math functions of host and device are good to a few ulp: below 1e-14 in all); a call on (first_chain, first_step)
    is the slice of the full table, bit for bit; host and device pointers give the same table."""
    import torch

    eng = _engine(qp, oracle, n)
    dim = 16**n
    for seed, c0 in ((DRAW_SEEDS[n], 0), (0xFEDCBA9876543210, (1 << 32) + 3)):
        deltas, uniforms = eng.mhmc_process_draws(seed, 4, 9, first_chain=c0)
        assert deltas.shape == (4, 9, dim) and uniforms.shape == (4, 9)
        want_d, want_u = host_draws(seed, c0, 4, 0, 9, dim)
        assert np.array_equal(uniforms, want_u)
        assert np.abs(deltas - want_d).max() < TOL
        part_d, part_u = eng.mhmc_process_draws(seed, 2, 5, first_chain=c0 + 1, first_step=3)
        assert np.array_equal(part_d, deltas[1:3, 3:8]) and np.array_equal(part_u, uniforms[1:3, 3:8])
    dev = torch.device("cuda", eng.device)
    out = (torch.empty((4, 9, dim), dtype=torch.float64, device=dev), torch.empty((4, 9), dtype=torch.float64, device=dev))
    eng.mhmc_process_draws(seed, 4, 9, first_chain=c0, out=out)
    eng.sync()
    assert np.array_equal(out[0].cpu().numpy(), deltas) and np.array_equal(out[1].cpu().numpy(), uniforms)
    assert eng.mhmc_process_draws(seed, 0, 9)[0].shape == (0, 9, dim)  # C = 0: nothing to do
    with pytest.raises(qp.engine.EngineError) as e:
        eng.mhmc_process_draws(seed, 1, 4, first_step=2**32 - 4)  # a step beyond 2^32 - 2
    assert e.value.code == qp._capi.QT_ERR_ARG


# ---- 2. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("n,chains", cases.CASES)
def test_fused_chain_equals_the_unfused_composition(qp, oracle, n, chains, setting):
    burn, n_points, thinning = SETTINGS[setting]
    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    want_dist, want_acc, thr = _reference(qp, oracle, n, chains, setting)
    eng = _engine(qp, oracle, n)
    hits, acc, dist = eng.mhmc_process_hits(counts, x0, x0, thr, DRAW_SEEDS[n], burn, n_points, thinning, cases.STEPS[n],
                                            return_dist=True)
    share = want_acc.sum() / (chains * n_points * thinning)
    err = np.abs(dist - want_dist).max()
    close = np.abs(thr[:, None] - want_dist) <= TOL
    lo = (thr[:, None] > want_dist + TOL).sum(axis=1)
    hi = (thr[:, None] > want_dist - TOL).sum(axis=1)
    print(f"n={n} C={chains} {setting}: acceptance share {share:.3f}, max |dist - unfused| {err:.2e}, hits {hits.tolist()} "
          f"in [{lo.tolist()}, {hi.tolist()}], accepted {acc.tolist()} / unfused {want_acc.tolist()}")
    assert hits.dtype == np.int64 and acc.dtype == np.int64 and dist.shape == (chains, n_points)
    assert np.array_equal(acc, want_acc)
    assert err < TOL
    assert close.mean() == 0.0  # a condition on the inputs: no distance within 1e-13 of its threshold, so hits is pinned
    assert np.array_equal(lo, hi) and np.all(lo <= hits) and np.all(hits <= hi)
    assert 0 < hits.sum() < chains * n_points  # both outcomes of the comparison occur
    assert 0.05 < share < 0.95  # both branches of the step run


# ---- 3. position independence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chains,first", [(1, 5, 2), (2, 3, 1)])
def test_chains_do_not_depend_on_their_place_in_the_batch(qp, oracle, n, chains, first):
    """Chains [first, C) computed alone with first_chain = first: the bits of those rows of the whole batch's call."""
    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    eng = _engine(qp, oracle, n)
    for setting in sorted(SETTINGS):
        thr = _reference(qp, oracle, n, chains, setting)[2]
        args = (DRAW_SEEDS[n], *SETTINGS[setting], cases.STEPS[n])
        full = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True)
        part = eng.mhmc_process_hits(counts[first:], x0[first:], x0[first:], thr[first:], *args, first_chain=first,
                                     return_dist=True)
        for a, b in zip(full, part):
            assert np.array_equal(a[first:], b), (n, setting)
        shifted = eng.mhmc_process_hits(counts[first:], x0[first:], x0[first:], thr[first:], *args, return_dist=True)
        assert not np.array_equal(shifted[2], part[2])  # (other numbers: first_chain is what keys them)


# ---- 4. pointers and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chains", [(1, 5), (2, 3)])
def test_pointer_kinds_and_edges(qp, oracle, n, chains):
    import torch

    povm, ins, counts, chois, x0 = _batch(oracle, n, chains)
    eng = _engine(qp, oracle, n)
    thr = _reference(qp, oracle, n, chains, "thinned")[2]
    seed, step = DRAW_SEEDS[n], cases.STEPS[n]
    args = (seed, *SETTINGS["thinned"], step)
    hits, acc, dist = eng.mhmc_process_hits(counts, x0, x0, thr, *args, return_dist=True)
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, x0, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_process_hits(*on_dev, *args, return_dist=True)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_process_hits(counts, x0, x0, thr, *args)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN threshold never counts
    nan_hits, nan_acc = eng.mhmc_process_hits(counts, x0, x0, np.full(chains, np.nan), *args)
    assert not nan_hits.any() and np.array_equal(nan_acc, acc)
    # C = 0
    empty = eng.mhmc_process_hits(counts[:0], x0[:0], x0[:0], thr[:0], *args, return_dist=True)
    assert [a.shape for a in empty] == [(0,), (0,), (0, SETTINGS["thinned"][1])]
    # argument errors of the entry: thinning < 1, burn_steps < 0, burn_steps + n_points * thinning >= 2^32 - 1
    for bad in ((seed, 3, 7, 0, step), (seed, -1, 7, 1, step), (seed, 2**31 - 1, 2**31 - 1, 2, step)):
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_process_hits(counts, x0, x0, thr, *bad)
        assert e.value.code == qp._capi.QT_ERR_ARG
    with pytest.raises(qp.engine.EngineError) as e:
        eng.mhmc_process_hits(counts, x0, x0, thr, seed, 3, -1, 1, step)  # n_points < 0
    assert e.value.code == qp._capi.QT_ERR_ARG


def test_three_qubits_are_refused_without_a_launch(qp):
    from quantpy_amd import _capi

    eng = qp.get_engine(3)  # (whatever is registered on it: the refusal comes first)
    one = np.zeros(1, dtype=np.int64)
    code = eng.lib.qt_mhmc_process_draws(eng._h, 1, 0, 1, 0, 1, one.ctypes.data, one.ctypes.data, _capi.QT_HOST_PTR)
    assert code == _capi.QT_ERR_UNSUPPORTED and "n_qubits 1..2" in _capi.last_error()
    code = eng.lib.qt_mhmc_process_hits(eng._h, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, 0,
                                        1, 1, 0.1, one.ctypes.data, one.ctypes.data, None, _capi.QT_HOST_PTR)
    assert code == _capi.QT_ERR_UNSUPPORTED and "n_qubits 1..2" in _capi.last_error()


def test_entries_need_the_povm_and_the_process_setup(qp):
    """A fresh handle: QT_ERR_STATE, the error the other process entries give, and nothing is launched."""
    from quantpy_amd import _capi

    eng = qp.engine.Engine(1)
    one = np.zeros(1, dtype=np.int64)

    def both():
        yield eng.lib.qt_mhmc_process_draws(eng._h, 1, 0, 1, 0, 1, one.ctypes.data, one.ctypes.data, _capi.QT_HOST_PTR)
        yield eng.lib.qt_mhmc_process_hits(eng._h, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0,
                                           0, 1, 1, 0.1, one.ctypes.data, one.ctypes.data, None, _capi.QT_HOST_PTR)

    try:
        for code in both():
            assert code == _capi.QT_ERR_STATE and "qt_set_povm" in _capi.last_error()
        eng.set_povm(qp.generate_measurement_matrix("proj-set", 1), np.ones(3) * 1000)
        for code in both():
            assert code == _capi.QT_ERR_STATE and "qt_process_setup" in _capi.last_error()
    finally:
        eng.close()


# ---- 5. the public function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_study_reproduces_its_hits_through_the_unfused_path(qp, n):
    from quantpy_amd import metrics

    channel = qp.channel.depolarizing(0.2, n)
    n_iter, n_points, burn = 4, 7, 3
    step = cases.STEPS[n]
    kw = dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, step=step, n_measurements=cases.SHOTS, sampler="numpy",
              seed=60 + n)
    np.random.seed(400 + n)
    out = metrics.get_CL_list_channel_mhmc(channel, return_details=True, **kw)
    assert out["seed"] == 61 + n and out["counts"].shape[0] == n_iter
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    tmg.experiment_batch(cases.SHOTS, "proj-set", repeats=1)  # (registers the POVM and the shots on the tomograph)
    eng = tmg._engine()
    dist, acc = unfused(eng, out["counts"], out["estimates"], out["seed"], burn, n_points, 1, step)
    assert not (np.abs(out["delta"][:, None] - dist) <= TOL).any()  # the condition that pins the hits
    hits = (out["delta"][:, None] > dist).sum(axis=1)
    print(f"n={n} study: hits {out['hits'].tolist()} / unfused {hits.tolist()}, accepted {acc.tolist()}")
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["acceptance_rate"], acc / n_points)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    assert np.array_equal(out["delta"], eng.hs_dist(out["estimates"], channel.choi.matrix))
    np.random.seed(400 + n)
    assert np.array_equal(metrics.get_CL_list_channel_mhmc(channel, **kw), np.sort(out["levels"]))


def test_study_refuses_a_three_qubit_channel(qp):
    from quantpy_amd import metrics

    with pytest.raises(NotImplementedError, match="one and two qubits"):
        metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1)
