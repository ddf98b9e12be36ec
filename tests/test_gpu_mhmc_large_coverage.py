"""GPU: the chain coverage study at n = 4, 5 -- qt_mhmc_draws_dim, qt_mhmc_state_large_hits,
qt_mhmc_state_large_metric_hits, metrics.get_CL_list_state_mhmc on four- and five-qubit states.

Inputs (tests/mhmc_large_coverage_cases.py): mixed_ghz(n, 0.5), 'proj-set', three experiments per size at 10 000 (n = 4)
and 100 000 (n = 5) shots per setting, STEP = 2.0, settings (burn_steps, n_points, thinning) = (3, 20, 2) and (0, 60, 1),
cases C = 1 (the first experiment) and C = 3.  Philox seeds and the rejected post-burn steps per chain of the CPU oracle
on host-built draws:
    n = 4, seed 3006: (3, 20, 2) -> [2, 1, 1],  (0, 60, 1) -> [3, 1, 1]
    n = 5, seed 3023: (3, 20, 2) -> [1, 1, 1],  (0, 60, 1) -> [1, 2, 1]
The condition -- every chain rejects at least one post-burn step and accepts at least one -- is asserted on the device's
own unfused run.

The fused kernels are compared with the UNFUSED composition of entries that predate them plus qt_mhmc_draws_dim: the
draws fed to qt_mhmc_state (k_mhmc_state_large), the kept states chain[:, burn::thinning][:, :n_points] through
qt_chol_unparam and qt_hs_dist_dim / qt_metric_dist_dim.  `accepted` must be equal as integers; a distance lies within
TOL_n = 10 d^2 eps of the unfused one (FP64 sums of at most d^2 terms of magnitude <= 1: 5.7e-13 at n = 4, 2.3e-12 at
n = 5).  For 'trace' / 'if' both sides run the same device functions on the same inputs: the design target is equal
bits, printed with the maximum difference."""
import numpy as np
import pytest

import mhmc_coverage_cases as small
import mhmc_large_coverage_cases as cases

pytestmark = pytest.mark.gpu

STEP = cases.STEP
SETTINGS = cases.SETTINGS
CASES = [(4, 1), (4, 3), (5, 1), (5, 3)]
METRICS = [None, "trace", "if"]  # None: Hilbert-Schmidt
DRAW_TOL = 1e-13


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return small.build_host_draws(tmp_path_factory.mktemp("mhmc_draws"))


def _engine(qp, n):
    eng = qp.get_engine(n)  # (the cached engine of this size: other tests register their own POVM)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * cases.SHOTS[n])
    return eng


_BATCHES, _CHAINS, _UNFUSED = {}, {}, {}


def _batch(qp, oracle, n, chains):
    """(counts, estimates, true state, x0) of a case, computed once: the first `chains` of the size's experiments."""
    if n not in _BATCHES:
        counts, rho = cases.trial_counts(oracle, n)
        assert cases.smallest_eigenvalues(oracle, n, counts).min() > 1e-3  # the CPU oracle: positive definite estimates
        eng = _engine(qp, n)
        est = eng.lin(counts)
        x0, status = eng.chol_param(est)
        assert not status.any()
        for a in (counts, est, x0):
            a.setflags(write=False)
        _BATCHES[n] = counts, est, rho, x0
    counts, est, rho, x0 = _BATCHES[n]
    return counts[:chains], est[:chains], rho, x0[:chains]


def _delta(eng, est, rho, metric):
    return eng.hs_dist(est, rho) if metric is None else eng.metric_dist_dim(est, rho, metric)


def _reference(qp, oracle, n, chains, setting, metric):
    """(unfused distances, unfused accepted, thresholds), computed once: the thresholds are the trial's own delta in
    `metric` for the odd chains and the nudged median of the chain's unfused distances for the even ones."""
    key = (n, chains, setting, metric)
    if key not in _UNFUSED:
        counts, est, rho, x0 = _batch(qp, oracle, n, chains)
        eng = _engine(qp, n)
        if key[:3] not in _CHAINS:
            _CHAINS[key[:3]] = cases.kept_states(eng, counts, x0, cases.DRAW_SEEDS[n], *SETTINGS[setting], STEP)
        mats, acc = _CHAINS[key[:3]]
        dist = cases.unfused_dist(eng, mats, est, metric)
        delta = _delta(eng, est, rho, metric)
        thr = np.array([delta[c] if c % 2 else cases.median_off_samples(dist[c]) for c in range(chains)])
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _UNFUSED[key] = dist, acc, thr
    return _UNFUSED[key]


# ---- 1. the draws ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_draws_dim_are_the_draws_of_the_small_handles(qp, n):
    eng = qp.get_engine(n)
    for seed, c0, s0 in ((cases.DRAW_SEEDS[4], 0, 0), (0xFEDCBA9876543210, (1 << 32) + 3, 5)):
        want = eng.mhmc_draws(seed, 4, 9, first_chain=c0, first_step=s0)
        got = eng.mhmc_draws_dim(4**n, seed, 4, 9, first_chain=c0, first_step=s0)
        assert got[0].shape == (4, 9, 4**n) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("n", [4, 5])
def test_draws_dim_are_the_host_functions(qp, host_draws, n):
    """Uniforms bit for bit, increments to 1e-13 absolute (|r| <= 8.6, the argument 2 pi u2 rounds to <= 6.3 eps, the
    math functions of host and device are good to a few ulp: below 1e-14 in all); a call on (first_chain, first_step)
    is the slice of the full table, bit for bit; host and device pointers give the same table."""
    import torch

    from quantpy_amd import _capi

    eng = qp.get_engine(n)  # (no POVM is read)
    dim = 4**n
    for seed, c0 in ((cases.DRAW_SEEDS[n], 0), (0xFEDCBA9876543210, (1 << 32) + 3)):
        deltas, uniforms = eng.mhmc_draws_dim(dim, seed, 4, 9, first_chain=c0)
        want_d, want_u = host_draws(seed, c0, 4, 0, 9, dim)
        assert np.array_equal(uniforms, want_u)
        assert np.abs(deltas - want_d).max() < DRAW_TOL
        part_d, part_u = eng.mhmc_draws_dim(dim, seed, 2, 5, first_chain=c0 + 1, first_step=3)
        assert np.array_equal(part_d, deltas[1:3, 3:8]) and np.array_equal(part_u, uniforms[1:3, 3:8])
    dev = torch.device("cuda", eng.device)
    out = (torch.empty((4, 9, dim), dtype=torch.float64, device=dev), torch.empty((4, 9), dtype=torch.float64, device=dev))
    eng.mhmc_draws_dim(dim, seed, 4, 9, first_chain=c0, out=out)
    eng.sync()
    assert np.array_equal(out[0].cpu().numpy(), deltas) and np.array_equal(out[1].cpu().numpy(), uniforms)
    assert eng.mhmc_draws_dim(dim, seed, 0, 9)[0].shape == (0, 9, dim)  # C = 0: nothing to do
    wrong = [dict(dim=dim + 1), dict(dim=0), dict(dim=-2), dict(dim=4098), dict(first_step=2**32 - 4), dict(chains=-1)]
    for kw in wrong:
        args = dict(dim=dim, seed=seed, chains=1, steps=4)
        args.update(kw)
        if args["chains"] < 0:  # (no NumPy array of that shape: the entry itself)
            one = np.zeros(1)
            rc = eng.lib.qt_mhmc_draws_dim(eng._h, dim, seed, 0, -1, 0, 4, one.ctypes.data, one.ctypes.data, _capi.QT_HOST_PTR)
            assert rc == _capi.QT_ERR_ARG
            continue
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_draws_dim(**args)
        assert e.value.code == _capi.QT_ERR_ARG, kw
    rc = eng.lib.qt_mhmc_draws_dim(eng._h, dim, seed, 0, 1, 0, 4, None, None, _capi.QT_HOST_PTR)
    assert rc == _capi.QT_ERR_ARG


# ---- 2. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("n,chains", CASES)
def test_fused_chain_equals_the_unfused_composition(qp, oracle, n, chains, setting):
    burn, n_points, thinning = SETTINGS[setting]
    counts, est, rho, x0 = _batch(qp, oracle, n, chains)
    eng = _engine(qp, n)
    tol = cases.tol(n)
    args = (cases.DRAW_SEEDS[n], burn, n_points, thinning, STEP)
    accepted = {}
    for metric in METRICS:
        want_dist, want_acc, thr = _reference(qp, oracle, n, chains, setting, metric)
        hits, acc, dist = eng.mhmc_state_large_hits(counts, est, x0, thr, *args, return_dist=True, metric=metric)
        err = np.abs(dist - want_dist).max()
        lo = (thr[:, None] > want_dist + tol).sum(axis=1)
        hi = (thr[:, None] > want_dist - tol).sum(axis=1)
        print(f"n={n} C={chains} {metric or 'hs'} {setting}: max |dist - unfused| {err:.2e} (bit-equal: "
              f"{np.array_equal(dist, want_dist)}), distances in [{want_dist.min():.3e}, {want_dist.max():.3e}], hits "
              f"{hits.tolist()} in [{lo.tolist()}, {hi.tolist()}], accepted {acc.tolist()} / unfused {want_acc.tolist()} of "
              f"{n_points * thinning}")
        assert hits.dtype == np.int64 and acc.dtype == np.int64 and dist.shape == (chains, n_points)
        # the condition on the inputs: every chain rejects at least one post-burn step and accepts at least one
        assert np.all(want_acc >= 1) and np.all(want_acc <= n_points * thinning - 1)
        assert np.array_equal(acc, want_acc)
        assert err < tol
        assert not (np.abs(thr[:, None] - want_dist) <= tol).any()  # the condition on the inputs that pins the hits
        assert np.array_equal(lo, hi) and np.array_equal(hits, lo)
        assert 0 < hits.sum() < chains * n_points  # both outcomes of the comparison occur
        accepted[metric] = acc
    assert np.array_equal(accepted[None], accepted["trace"]) and np.array_equal(accepted[None], accepted["if"])


# ---- 3. seams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", [4, 5])
def test_seams(qp, oracle, n, metric):
    import torch

    from quantpy_amd import _capi

    counts, est, rho, x0 = _batch(qp, oracle, n, 3)
    eng = _engine(qp, n)
    thr = _reference(qp, oracle, n, 3, "thinned", metric)[2]
    n_points = SETTINGS["thinned"][1]
    args = (cases.DRAW_SEEDS[n], *SETTINGS["thinned"], STEP)
    hits, acc, dist = eng.mhmc_state_large_hits(counts, est, x0, thr, *args, return_dist=True, metric=metric)
    # chains [1, 3) alone with first_chain = 1: rows 1..2 of the C = 3 call
    part = eng.mhmc_state_large_hits(counts[1:], est[1:], x0[1:], thr[1:], *args, first_chain=1, return_dist=True, metric=metric)
    for a, b in zip((hits, acc, dist), part):
        assert np.array_equal(a[1:], b)
    # torch tensors
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, est, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_state_large_hits(*on_dev, *args, return_dist=True, metric=metric)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_state_large_hits(counts, est, x0, thr, *args, metric=metric)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN threshold never counts
    nan_thr = np.array(thr)
    nan_thr[1] = np.nan
    n_hits, n_acc = eng.mhmc_state_large_hits(counts, est, x0, nan_thr, *args, metric=metric)
    assert n_hits[1] == 0 and np.array_equal(n_hits[[0, 2]], hits[[0, 2]]) and np.array_equal(n_acc, acc)
    # C = 0
    empty = eng.mhmc_state_large_hits(counts[:0], est[:0], x0[:0], thr[:0], *args, return_dist=True, metric=metric)
    assert [a.shape for a in empty] == [(0,), (0,), (0, n_points)]
    # the argument errors of qt_mhmc_state_hits
    seed = cases.DRAW_SEEDS[n]
    for wrong in ((seed, 3, 20, 0, STEP), (seed, -1, 20, 1, STEP), (seed, 2**31 - 1, 2**31 - 1, 2, STEP),
                  (seed, 1, 2**31 - 1, 2, STEP)):  # the last: burn_steps + n_points * thinning = 2^32 - 1
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_state_large_hits(counts, est, x0, thr, *wrong, metric=metric)
        assert e.value.code == _capi.QT_ERR_ARG, wrong


def test_three_qubits_are_refused_and_sent_to_the_existing_entry(qp):
    from quantpy_amd import _capi

    eng = qp.get_engine(3)  # (no POVM registered: the refusal comes first)
    one = np.zeros(1, dtype=np.int64)
    tail = (one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, 0, 1, 1, 0.1, one.ctypes.data,
            one.ctypes.data, None, _capi.QT_HOST_PTR)
    assert eng.lib.qt_mhmc_state_large_hits(eng._h, *tail) == _capi.QT_ERR_UNSUPPORTED
    assert "qt_mhmc_state_hits" in _capi.last_error()
    assert eng.lib.qt_mhmc_state_large_metric_hits(eng._h, _capi.QT_METRIC_TRACE, *tail) == _capi.QT_ERR_UNSUPPORTED
    assert "qt_mhmc_state_metric_hits" in _capi.last_error()


# ---- 4. the public function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_iter", [(4, 3), (5, 2)])
def test_study_runs_at_four_and_five_qubits(qp, n, n_iter):
    from quantpy_amd import geometry, metrics

    state = qp.Qobj(small.mixed_ghz(n))
    n_points, burn, thinning = 20, 3, 2
    kw = dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, thinning=thinning, n_measurements=cases.SHOTS[n], step=STEP,
              seed=60 + n, return_details=True)
    outs = {dst: metrics.get_CL_list_state_mhmc(state, dst=dst, **kw) for dst in ("hs", "trace", "if")}
    eng = _engine(qp, n)
    for dst, out in outs.items():
        metric = None if dst == "hs" else dst
        assert out["counts"].shape[0] == n_iter and out["levels"].shape == (n_iter,)
        assert np.array_equal(out["counts"], outs["hs"]["counts"]) and np.array_equal(out["estimates"], outs["hs"]["estimates"])
        x0, status = eng.chol_param(out["estimates"])
        assert not status.any()
        delta = _delta(eng, out["estimates"], state.matrix, metric)
        assert np.array_equal(out["delta"], delta)
        hits, acc = eng.mhmc_state_large_hits(out["counts"], out["estimates"], x0, delta, out["seed"], burn, n_points, thinning,
                                              STEP, metric=metric)
        print(f"n={n} {dst}: delta {delta.tolist()}, hits {hits.tolist()}, accepted {acc.tolist()}")
        assert np.array_equal(out["hits"], hits)
        assert np.array_equal(out["acceptance_rate"], acc / (n_points * thinning))
        assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
        assert np.array_equal(out["acceptance_rate"], outs["hs"]["acceptance_rate"])  # the chains do not depend on the distance
    # 'hs' as a string, as the function of quantpy_amd.geometry and by default
    for other in (metrics.get_CL_list_state_mhmc(state, dst=geometry.hs_dst, **kw), metrics.get_CL_list_state_mhmc(state, **kw)):
        assert sorted(other) == sorted(outs["hs"])
        for k in other:
            assert np.array_equal(other[k], outs["hs"][k]), k
    # at 1000 shots per setting the 'lin' estimates are not positive definite: no chain to start
    kw["n_measurements"] = 1000
    with pytest.raises(np.linalg.LinAlgError):
        metrics.get_CL_list_state_mhmc(state, **kw)
