"""GPU: the chain coverage study -- qt_mhmc_draws, qt_mhmc_state_hits, metrics.get_CL_list_state_mhmc.

Batches: n = 1 with C = 5 and 17 chains (16 per wavefront: a partial group and one that spills into a second wavefront),
n = 2 with C = 5, n = 3 with C = 1 and 5 (the last workgroup of four wavefronts is padded); two step settings,
(burn_steps, n_points, thinning) = (3, 7, 2) and (0, 40, 1).  Every chain has its own counts: 1000 shots per setting of
the GHZ state mixed half-and-half with the identity, on np.random's stream; the 'lin' estimates of these counts are all
positive definite (asserted from the CPU oracle below), and each chain starts at the Cholesky factor of its own.

The fused kernel is compared with the UNFUSED composition of entries that predate it: the draws dumped by qt_mhmc_draws
fed to qt_mhmc_state, the kept states through qt_chol_unparam and qt_hs_dist_dim.  Tolerance of a distance, 1e-13
absolute: both sides are FP64 sums of at most 64 terms of magnitude <= 1, error about d^2 eps = 7e-15, times ten.

STEP = 2.0 and the Philox seeds of the draws were chosen by running the unfused path (on the CPU oracle, with the host
instantiation of the draws): the reference's target is exp(-nll) with the frequencies normalised to sum 1, so flat that
most proposals are accepted whatever the step (n = 3: about 3.5 % rejected per step for every step from 0.2 to 6, fewer
below).  The condition `0.05 < acceptance share < 0.95` therefore needs a seed whose uniforms reject often enough; for
n = 3 it is 7581, the first of 3000, 3001, ... at which all four n = 3 cases stay below 0.915, so that each case has
three to seven rejections more than the bound asks for (a change of the draws' definition or of the nll arithmetic needs
a new search).  Acceptance shares of that run, settings (3, 7, 2) / (0, 40, 1):
    n = 1, C = 5: 0.829 / 0.865     n = 1, C = 17: 0.832 / 0.859     n = 2, C = 5: 0.929 / 0.905
    n = 3, C = 1: 0.714 / 0.850     n = 3, C = 5: 0.843 / 0.910
The test asserts the condition on the device's own unfused run."""
import numpy as np
import pytest

import mhmc_coverage_cases as cases

pytestmark = pytest.mark.gpu

STEP = 2.0
TOL = 1e-13
SETTINGS = {"thinned": (3, 7, 2), "plain": (0, 40, 1)}  # burn_steps, n_points, thinning
CASES = [(1, 5), (1, 17), (2, 5), (3, 1), (3, 5)]


DRAW_SEEDS = {1: 2025, 2: 2026, 3: 7581}  # Philox seeds of the chains (module docstring)


def _draw_seed(n):
    return DRAW_SEEDS[n]


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


@pytest.fixture(scope="module")
def host_draws(tmp_path_factory):
    return cases.build_host_draws(tmp_path_factory.mktemp("mhmc_draws"))


def _engine(qp, n):
    eng = qp.get_engine(n)  # (the cached engine of this size: other tests register their own POVM)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * cases.SHOTS)
    return eng


_BATCHES, _UNFUSED = {}, {}


def _batch(qp, oracle, n, chains):
    """(counts, estimates, delta, x0) of a case, computed once."""
    if (n, chains) not in _BATCHES:
        counts, rho = cases.trial_counts(oracle, n, chains, 100 * n + chains)
        povm = oracle.measurement_matrix("proj-set", n)
        for c in counts:  # the CPU oracle: every unclipped 'lin' estimate is positive definite
            assert np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)).min() > 1e-3
        eng = _engine(qp, n)
        est = eng.lin(counts)
        x0, status = eng.chol_param(est)
        assert not status.any()
        _BATCHES[n, chains] = counts, est, eng.hs_dist(est, rho), x0
    return _BATCHES[n, chains]


def unfused(eng, counts, centres, x0, seed, burn, n_points, thinning, step, first_chain=0):
    """The study's chain on entries that predate the fused kernel: (kept distances (C, n_points), accepted post-burn
    steps (C,))."""
    chains, total = counts.shape[0], burn + n_points * thinning
    deltas, uniforms = eng.mhmc_draws(seed, chains, total, first_chain=first_chain)
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, step)
    kept = chain[:, burn::thinning][:, :n_points]
    mats = eng.chol_unparam(kept.reshape(-1, eng.D)).reshape(chains, n_points, eng.d, eng.d)
    dist = np.stack([eng.hs_dist(mats[c], centres[c]) for c in range(chains)])
    return dist, acc[:, burn:].sum(axis=1).astype(np.int64)


def _median_off_samples(dist):
    """A threshold in the middle of one chain's distances and on none of them."""
    s = np.unique(dist)
    return 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) > 1 else 1.5 * s[0] + 1e-3


def _reference(qp, oracle, n, chains, setting):
    """(unfused distances, unfused accepted, thresholds) of a case and setting, computed once: the thresholds are the
    trial's own delta for the odd chains and the nudged median of the chain's unfused distances for the even ones."""
    key = (n, chains, setting)
    if key not in _UNFUSED:
        counts, est, delta, x0 = _batch(qp, oracle, n, chains)
        dist, acc = unfused(_engine(qp, n), counts, est, x0, _draw_seed(n), *SETTINGS[setting], STEP)
        thr = np.array([delta[c] if c % 2 else _median_off_samples(dist[c]) for c in range(chains)])
        for a in (dist, acc, thr):
            a.setflags(write=False)
        _UNFUSED[key] = dist, acc, thr
    return _UNFUSED[key]


# ---- 1. the draws against their definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_draws_are_the_host_functions(qp, host_draws, n):
    """Uniforms bit for bit, increments to 1e-13 absolute (|r| <= 8.6, the argument 2 pi u2 rounds to <= 6.3 eps, the
    math functions of host and device are good to a few ulp: below 1e-14 in all); a call on (first_chain, first_step)
    is the slice of the full table, bit for bit; host and device pointers give the same table."""
    import torch

    eng = qp.get_engine(n)
    dim = 4**n
    for seed, c0 in ((_draw_seed(n), 0), (0xFEDCBA9876543210, (1 << 32) + 3)):
        deltas, uniforms = eng.mhmc_draws(seed, 4, 9, first_chain=c0)
        want_d, want_u = host_draws(seed, c0, 4, 0, 9, dim)
        assert np.array_equal(uniforms, want_u)
        assert np.abs(deltas - want_d).max() < TOL
        part_d, part_u = eng.mhmc_draws(seed, 2, 5, first_chain=c0 + 1, first_step=3)
        assert np.array_equal(part_d, deltas[1:3, 3:8]) and np.array_equal(part_u, uniforms[1:3, 3:8])
    dev = torch.device("cuda", eng.device)
    out = (torch.empty((4, 9, dim), dtype=torch.float64, device=dev), torch.empty((4, 9), dtype=torch.float64, device=dev))
    eng.mhmc_draws(seed, 4, 9, first_chain=c0, out=out)
    eng.sync()
    assert np.array_equal(out[0].cpu().numpy(), deltas) and np.array_equal(out[1].cpu().numpy(), uniforms)
    assert eng.mhmc_draws(seed, 0, 9)[0].shape == (0, 9, dim)  # C = 0: nothing to do
    with pytest.raises(qp.engine.EngineError):
        eng.mhmc_draws(seed, 1, 4, first_step=2**32 - 4)  # a step beyond 2^32 - 2


# ---- 2. fused against unfused ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("n,chains", CASES)
def test_fused_chain_equals_the_unfused_composition(qp, oracle, n, chains, setting):
    burn, n_points, thinning = SETTINGS[setting]
    counts, est, delta, x0 = _batch(qp, oracle, n, chains)
    want_dist, want_acc, thr = _reference(qp, oracle, n, chains, setting)
    eng = _engine(qp, n)
    hits, acc, dist = eng.mhmc_state_hits(counts, est, x0, thr, _draw_seed(n), burn, n_points, thinning, STEP, return_dist=True)
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
@pytest.mark.parametrize("n", [1, 3])
def test_chains_do_not_depend_on_their_place_in_the_batch(qp, oracle, n):
    """Chains [2, 5) computed alone with first_chain = 2: the bits of rows 2..4 of the C = 5 call."""
    counts, est, delta, x0 = _batch(qp, oracle, n, 5)
    eng = _engine(qp, n)
    for setting in sorted(SETTINGS):
        thr = _reference(qp, oracle, n, 5, setting)[2]
        args = (_draw_seed(n), *SETTINGS[setting], STEP)
        full = eng.mhmc_state_hits(counts, est, x0, thr, *args, return_dist=True)
        part = eng.mhmc_state_hits(counts[2:], est[2:], x0[2:], thr[2:], *args, first_chain=2, return_dist=True)
        for a, b in zip(full, part):
            assert np.array_equal(a[2:], b), (n, setting)
        shifted = eng.mhmc_state_hits(counts[2:], est[2:], x0[2:], thr[2:], *args, return_dist=True)
        assert not np.array_equal(shifted[2], part[2])  # (other numbers: first_chain is what keys them)


# ---- 4. pointers and edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_pointer_kinds_and_edges(qp, oracle, n):
    import torch

    counts, est, delta, x0 = _batch(qp, oracle, n, 5)
    eng = _engine(qp, n)
    thr = _reference(qp, oracle, n, 5, "thinned")[2]
    args = (_draw_seed(n), *SETTINGS["thinned"], STEP)
    hits, acc, dist = eng.mhmc_state_hits(counts, est, x0, thr, *args, return_dist=True)
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.array(a)).to(dev) for a in (counts, est, x0, thr)]
    d_hits, d_acc, d_dist = eng.mhmc_state_hits(*on_dev, *args, return_dist=True)
    eng.sync()
    assert np.array_equal(d_hits.cpu().numpy(), hits) and np.array_equal(d_acc.cpu().numpy(), acc)
    assert np.array_equal(d_dist.cpu().numpy(), dist)
    # dist = NULL
    no_dist = eng.mhmc_state_hits(counts, est, x0, thr, *args)
    assert len(no_dist) == 2 and np.array_equal(no_dist[0], hits) and np.array_equal(no_dist[1], acc)
    # a NaN threshold never counts
    nan_hits, nan_acc = eng.mhmc_state_hits(counts, est, x0, np.full(5, np.nan), *args)
    assert not nan_hits.any() and np.array_equal(nan_acc, acc)
    # C = 0
    empty = eng.mhmc_state_hits(counts[:0], est[:0], x0[:0], thr[:0], *args, return_dist=True)
    assert [a.shape for a in empty] == [(0,), (0,), (0, SETTINGS["thinned"][1])]
    # argument errors of the entry
    for bad in ((_draw_seed(n), 3, 7, 0, STEP), (_draw_seed(n), -1, 7, 1, STEP), (_draw_seed(n), 2**31 - 1, 2**31 - 1, 2, STEP)):
        with pytest.raises(qp.engine.EngineError) as e:
            eng.mhmc_state_hits(counts, est, x0, thr, *bad)
        assert e.value.code == qp._capi.QT_ERR_ARG


def test_four_qubits_are_refused_without_a_launch(qp):
    from quantpy_amd import _capi

    eng = qp.get_engine(4)  # (no POVM registered: the refusal comes first)
    with pytest.raises(qp.engine.EngineError, match="n_qubits 1..3") as e:
        eng.mhmc_draws(1, 2, 3)
    assert e.value.code == _capi.QT_ERR_UNSUPPORTED
    one = np.zeros(1, dtype=np.int64)
    code = eng.lib.qt_mhmc_state_hits(eng._h, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 0, 0, 1,
                                      1, 0.1, one.ctypes.data, one.ctypes.data, None, _capi.QT_HOST_PTR)
    assert code == _capi.QT_ERR_UNSUPPORTED and "n_qubits 1..3" in _capi.last_error()


# ---- 5. the public function ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2])
def test_study_reproduces_its_hits_through_the_unfused_path(qp, n):
    from quantpy_amd import metrics

    state = qp.Qobj(cases.mixed_ghz(n))
    n_iter, n_points, burn = 6, 7, 3
    kw = dict(n_iter=n_iter, n_points=n_points, burn_steps=burn, step=STEP, sampler="numpy", seed=40 + n)
    np.random.seed(300 + n)
    out = metrics.get_CL_list_state_mhmc(state, return_details=True, **kw)
    assert out["seed"] == 41 + n and out["counts"].shape[0] == n_iter
    tmg = qp.StateTomograph(state)
    tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", n)
    tmg.n_measurements = np.ones(tmg.povm_matrix.shape[0]) * 1000
    eng = tmg._engine()
    x0, status = eng.chol_param(out["estimates"])
    assert not status.any()
    dist, acc = unfused(eng, out["counts"], out["estimates"], x0, out["seed"], burn, n_points, 1, STEP)
    assert not (np.abs(out["delta"][:, None] - dist) <= TOL).any()  # the condition that pins the hits
    hits = (out["delta"][:, None] > dist).sum(axis=1)
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["acceptance_rate"], acc / n_points)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    assert np.array_equal(out["delta"], eng.hs_dist(out["estimates"], state.matrix))
    np.random.seed(300 + n)
    assert np.array_equal(metrics.get_CL_list_state_mhmc(state, **kw), np.sort(out["levels"]))


def test_study_refuses_estimates_without_a_cholesky_factor(qp):
    """A pure GHZ state with method='lin': the clipped estimates are rank deficient up to the clip's 1e-15, and the study
    refuses them whichever way the factorisation's last pivots round (qt_chol_param itself takes them: status 0 on 1080
    of 1080 such trials)."""
    from quantpy_amd import metrics

    pure = qp.Qobj(cases.mixed_ghz(2, 1.0))
    with pytest.raises(np.linalg.LinAlgError):
        metrics.get_CL_list_state_mhmc(pure, n_iter=6, n_points=7, burn_steps=3, method="lin", seed=5)


def test_study_raises_on_a_trial_that_is_not_positive_definite(qp, monkeypatch):
    """The same study with the clip switched off underneath it: the raw linear inversion of a pure state has negative
    eigenvalues (qt_chol_param reports status 1), and the study raises before any chain runs."""
    from quantpy_amd import metrics

    clipped = qp.StateTomograph.point_estimate_batch

    def unclipped(self, counts, method="lin", **kw):
        kw["physical"] = False
        return clipped(self, counts, method=method, **kw)

    monkeypatch.setattr(qp.StateTomograph, "point_estimate_batch", unclipped)
    pure = qp.Qobj(cases.mixed_ghz(2, 1.0))
    with pytest.raises(np.linalg.LinAlgError, match="not positive definite"):
        metrics.get_CL_list_state_mhmc(pure, n_iter=6, n_points=7, burn_steps=3, method="lin", seed=5)
