"""GPU: the bootstrap coverage study (quantpy_amd.metrics, reference metrics.py:125-144) and what it is made of.

* qt_lin_dist_group_batch / qt_mle_dist_group_batch measure trial b of a resample-major batch against centre b % G.  The
  arithmetic is that of the ungrouped entries and only the centre's address differs, so `dist`, `status` and `nit` are
  compared BIT FOR BIT with G calls of qt_lin_dist_batch / qt_mle_dist_batch on counts[:, t] with centre t.  Shapes: G = 5
  centres, R = 7 resamples (B = 35: at n = 1 and n = 2 a wavefront holds 16 and 4 trials of different groups, at n = 3 one;
  35 is no multiple of a workgroup's trials at any n), and G = 3, R = 2 at n = 4.
* qt_group_hits against (thr[None, :] > dist).sum(0).
* get_CL_list_state with interval='boot' against the documented keying, redrawn resample by resample with the ungrouped
  sampler and estimators; interval='gamma' (state and channel) against MomentInterval plus the rule applied here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G, R = 5, 7
SHOTS = 100  # per setting: low enough that the linear inversion of a pure state needs the clip


def _states(n, count, seed):
    """`count` density matrices of n qubits: pure ones first (their estimates leave the cone), then mixed ones."""
    g = np.random.default_rng(seed)
    d = 2**n
    out = []
    for k in range(count):
        rank = 1 if k < (count + 1) // 2 else d
        m = g.standard_normal((d, rank)) + 1j * g.standard_normal((d, rank))
        rho = m @ m.conj().T
        out.append(rho / np.trace(rho).real)
    return np.stack(out)


def _case(n, groups, resamples, seed):
    """An engine with the 'proj-set' POVM and counts[R][G][S][K]: host multinomials around `groups` different states."""
    import quantpy_amd as qp
    from quantpy_amd.tomography.state import born_probabilities

    tensor = qp.generate_measurement_matrix("proj-set", n)  # (carries its one-qubit factor: the product form)
    povm = np.asarray(tensor)
    states = _states(n, groups, seed)
    g = np.random.default_rng(seed + 1)
    counts = np.empty((resamples, groups) + povm.shape[:2], dtype=np.int64)
    for t, rho in enumerate(states):
        p = born_probabilities(povm, qp.Qobj(rho).bloch)
        p /= p.sum(-1, keepdims=True)
        for r in range(resamples):
            counts[r, t] = [g.multinomial(SHOTS, ps) for ps in p]

    def engine():  # the cached engine of this size, with this case's POVM and shots (other tests register their own)
        eng = qp.get_engine(n)
        eng.set_povm(tensor, np.ones(povm.shape[0]) * SHOTS)
        return eng

    return engine, states, counts


@pytest.fixture(scope="module")
def cases():
    return {n: _case(n, G, R, 10 + n) for n in (1, 2, 3)}


def _clipped(eng, counts):
    """Trials whose unprojected linear inversion has a negative eigenvalue."""
    lin = eng.lin(counts.reshape((-1,) + counts.shape[2:]), physical=False)
    return np.linalg.eigvalsh(lin).min(-1) < 0


def _run(eng, method, counts, centre, **kw):
    """One device-pointer launch family: (dist, status, nit or None, helper-wave flag)."""
    import torch

    b = counts.shape[0]
    cd = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
    cen = torch.from_numpy(np.ascontiguousarray(centre, dtype=np.complex128)).cuda()
    dist = torch.full((b + 3,), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((b + 3,), -7, dtype=torch.int32, device="cuda")
    nit = torch.full((b + 3,), -7, dtype=torch.int32, device="cuda")
    if method == "lin":
        eng.lin_dist_dev(cd, cen, dist[:b], status=status[:b], **kw)
        helper = None
    else:
        eng.mle_dist_dev(cd, cen, dist[:b], status=status[:b], nit=nit[:b], **kw)
        helper = eng.mle_helper_wave
    eng.sync()
    dist, status, nit = dist.cpu().numpy(), status.cpu().numpy(), nit.cpu().numpy()
    assert (dist[b:] == -7.0).all() and (status[b:] == -7).all() and (nit[b:] == -7).all()  # nothing behind row B
    return dist[:b], status[:b], (nit[:b] if method == "mle" else None), helper


def _grouped_equals_ungrouped(eng, states, counts, method, **kw):
    resamples, groups = counts.shape[:2]
    flat = counts.reshape((resamples * groups,) + counts.shape[2:])  # resample-major: row r * G + t
    dist, status, nit, helper = _run(eng, method, flat, states, **kw)
    for t in range(groups):
        d1, s1, n1, h1 = _run(eng, method, counts[:, t], states[t], **kw)
        assert np.array_equal(dist.reshape(resamples, groups)[:, t].view(np.int64), d1.view(np.int64)), (t, dist, d1)
        assert np.array_equal(status.reshape(resamples, groups)[:, t], s1), (t, status, s1)
        if method == "mle":
            assert np.array_equal(nit.reshape(resamples, groups)[:, t], n1), (t, nit, n1)
            assert h1 == helper
    assert np.isfinite(dist).all() and (dist > 0).all()
    # the centres differ enough that a wrong one shows: trial t against centre t + 1 gives another distance
    other, *_ = _run(eng, method, counts[:, 0], states[1], **kw)
    assert not np.array_equal(other, dist.reshape(resamples, groups)[:, 0])
    return dist, helper


@pytest.mark.parametrize("physical", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_lin_grouped_centres(cases, n, physical):
    engine, states, counts = cases[n]
    eng = engine()
    assert _clipped(eng, counts).any()
    _grouped_equals_ungrouped(eng, states, counts, "lin", physical=physical)


# (helper wave, specialise, fused_max_waves or None for the default): every form of the MLE launch family
FORMS = [(1, 1, None), (0, 1, None), (1, 0, None), (0, 0, None), (1, 1, 0), (1, 0, 0)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("init", ["lin", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_mle_grouped_centres(cases, n, init, form):
    from quantpy_amd import _capi

    engine, states, counts = cases[n]
    eng = engine()
    helper_opt, spec, waves = form
    assert _clipped(eng, counts).any()
    try:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, helper_opt)
        eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, spec)
        if waves is not None:
            eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
        _, helper = _grouped_equals_ungrouped(eng, states, counts, "mle", init=init, max_iter=100, tol=1e-3)
        assert bool(eng.mle_specialised) == bool(spec)
    finally:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, 1)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    # the twin wavefronts run in the one-launch form at n = 3 from the 'lin' start, and nowhere else
    assert bool(helper) == (n == 3 and init == "lin" and helper_opt == 1 and waves is None)


def test_large_kernels_grouped_centres():
    engine, states, counts = _case(4, 3, 2, 40)
    eng = engine()
    assert _clipped(eng, counts).any()
    for physical in (True, False):
        _grouped_equals_ungrouped(eng, states, counts, "lin", physical=physical)
    _grouped_equals_ungrouped(eng, states, counts, "mle", init="lin", max_iter=30, tol=1e-3)


@pytest.mark.parametrize("n", [1, 3])
def test_one_group_is_the_old_entry(cases, n):
    """G = 1 through the new entries (a (1, d, d) table) equals qt_lin_dist_batch / qt_mle_dist_batch."""
    engine, states, counts = cases[n]
    eng = engine()
    flat = counts.reshape((-1,) + counts.shape[2:])
    for method, kw in (("lin", {}), ("mle", dict(init="lin")), ("mle", dict(init="mixed"))):
        new = _run(eng, method, flat, states[:1], **kw)
        old = _run(eng, method, flat, states[0], **kw)
        for a, b in zip(new[:3], old[:3]):
            assert (a is None and b is None) or np.array_equal(a, b)
        assert np.array_equal(new[0].view(np.int64), old[0].view(np.int64))


@pytest.mark.parametrize("n", [2, 3])
def test_host_pointer_calls_agree(cases, n):
    from quantpy_amd import _capi
    from quantpy_amd.engine import _ptr

    engine, states, counts = cases[n]
    eng = engine()
    flat = np.ascontiguousarray(counts.reshape((-1,) + counts.shape[2:]))
    cen = np.ascontiguousarray(states, dtype=np.complex128)
    b = flat.shape[0]
    for method in ("lin", "mle"):
        want = _run(eng, method, flat, states)
        dist, status, nit = np.empty(b), np.full(b, -1, dtype=np.int32), np.full(b, -1, dtype=np.int32)
        if method == "lin":
            rc = eng.lib.qt_lin_dist_group_batch(eng._h, _ptr(flat), b, 1, _ptr(cen), G, None, _ptr(dist), _ptr(status),
                                                 _capi.QT_HOST_PTR)
        else:
            rc = eng.lib.qt_mle_dist_group_batch(eng._h, _ptr(flat), b, _capi.QT_INIT_LIN, 100, 1e-3, _ptr(cen), G, None,
                                                 _ptr(dist), _ptr(nit), None, None, _ptr(status), _capi.QT_HOST_PTR)
        assert rc == 0, _capi.last_error()
        assert np.array_equal(dist.view(np.int64), want[0].view(np.int64)) and np.array_equal(status, want[1])
        if method == "mle":
            assert np.array_equal(nit, want[2])
    # argument errors of the new entries
    dist, status = np.empty(b), np.empty(b, dtype=np.int32)
    assert eng.lib.qt_lin_dist_group_batch(eng._h, _ptr(flat), b, 1, _ptr(cen), 0, None, _ptr(dist), _ptr(status), 0) == _capi.QT_ERR_ARG
    assert eng.lib.qt_lin_dist_group_batch(eng._h, _ptr(flat), b, 1, None, G, None, _ptr(dist), _ptr(status), 0) == _capi.QT_ERR_ARG
    assert eng.lib.qt_mle_dist_group_batch(eng._h, _ptr(flat), b, 0, 100, 1e-3, _ptr(cen), -1, None, _ptr(dist), None, None, None,
                                           _ptr(status), 0) == _capi.QT_ERR_ARG
    assert eng.lib.qt_mle_dist_group_batch(eng._h, _ptr(flat), b, 0, 100, 1e-3, None, G, None, _ptr(dist), None, None, None,
                                           _ptr(status), 0) == _capi.QT_ERR_ARG


# ---- qt_group_hits -------------------------------------------------------------------------------------------------------

def _hits_sample(r, g, seed):
    """dist (r, g) and thr (g,) with NaN, values equal to the threshold, and both zeros against a zero threshold."""
    rng = np.random.default_rng(seed)
    dist = rng.random((r, g))
    thr = rng.random(g)
    flat = dist.reshape(-1)
    pick = rng.permutation(flat.size)
    k = max(1, flat.size // 6)
    flat[pick[:k]] = np.nan
    eq = pick[k:2 * k]
    flat[eq] = np.tile(thr, r)[eq]  # equal to the column's threshold: does not count
    thr[0] = 0.0
    dist[:, 0] = np.where(rng.random(r) < 0.5, 0.0, -0.0)  # +-0.0 against 0.0: equal, does not count
    if g > 1:
        thr[g - 1] = np.nan  # a NaN threshold is above nothing
    return dist, thr


@pytest.mark.parametrize("shape", [(7, 5), (1, 1), (300, 3), (3, 300)])
def test_group_hits(shape):
    import torch

    import quantpy_amd as qp

    eng = qp.get_engine(1)
    r, g = shape
    dist, thr = _hits_sample(r, g, 3 * r + g)
    with np.errstate(invalid="ignore"):
        want = (thr[None, :] > dist).sum(0)
    assert g == 1 or want.max() > 0
    # host arrays, in place
    hits = np.zeros(g, dtype=np.int64)
    eng.group_hits(dist.reshape(-1), thr, hits)
    assert np.array_equal(hits, want)
    # device tensors; two accumulating calls over the rows equal one
    d_dist, d_thr = torch.from_numpy(dist).cuda(), torch.from_numpy(thr).cuda()
    one = torch.zeros(g, dtype=torch.int64, device="cuda")
    eng.group_hits(d_dist.reshape(-1), d_thr, one)
    two = torch.full((g + 2,), 11, dtype=torch.int64, device="cuda")
    cut = r // 2
    if cut:
        eng.group_hits(d_dist[:cut].reshape(-1), d_thr, two[:g])
    eng.group_hits(d_dist[cut:].reshape(-1), d_thr, two[:g])
    eng.sync()
    assert np.array_equal(one.cpu().numpy(), want)
    assert np.array_equal(two.cpu().numpy(), np.concatenate([want + 11, [11, 11]]))


def test_group_hits_needs_whole_resamples():
    import quantpy_amd as qp
    from quantpy_amd import _capi
    from quantpy_amd.engine import _ptr

    eng = qp.get_engine(1)
    dist, thr, hits = np.zeros(7), np.ones(3), np.zeros(3, dtype=np.int64)
    assert eng.lib.qt_group_hits(eng._h, _ptr(dist), 7, 3, _ptr(thr), _ptr(hits), 0) == _capi.QT_ERR_ARG
    assert eng.lib.qt_group_hits(eng._h, _ptr(dist), 6, 0, _ptr(thr), _ptr(hits), 0) == _capi.QT_ERR_ARG
    assert not hits.any()
    with pytest.raises(qp.EngineError):
        eng.group_hits(dist, thr, hits)


# ---- the study -----------------------------------------------------------------------------------------------------------

def _two_qubit_state():
    import quantpy_amd as qp

    return qp.qobj.GHZ(2)  # pure: at 100 shots per setting the linear inversion leaves the cone


@pytest.mark.parametrize("method_boot", ["lin", "mle"])
def test_boot_study_from_the_documented_keys(method_boot):
    """n = 2, n_iter = 3, n_points = 5: every resample redrawn from key `seed`, rows (r * 3 + t) * S .. + S, with the
    ungrouped sampler (period = S), reconstructed with point_estimate_batch and measured with hs_dist."""
    import quantpy_amd as qp
    from quantpy_amd import metrics

    state = _two_qubit_state()
    n_iter, n_points = 3, 5
    kw = dict(n_iter=n_iter, n_points=n_points, interval="boot", n_measurements=SHOTS, method="lin",
              method_boot=method_boot, seed=2024, return_details=True)
    out = metrics.get_CL_list_state(state, **kw)
    assert out["seed"] == 2025 and out["counts"].shape[0] == n_iter
    tmg = qp.StateTomograph(state)
    tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", 2)
    tmg.n_measurements = np.ones(tmg.povm_matrix.shape[0]) * SHOTS
    eng = tmg._engine()
    n_set = eng.S
    rho, _ = tmg.point_estimate_batch(out["counts"], method="lin")
    assert np.array_equal(rho, out["estimates"])
    delta = eng.hs_dist(rho, state.matrix)
    assert np.array_equal(delta, out["delta"])
    pvals = np.clip(eng.born_probs(eng.bloch_from_matrix(rho)), 0, 1)
    shots = np.full(n_set, SHOTS, dtype=np.int64)
    hits = np.zeros(n_iter, dtype=np.int64)
    for t in range(n_iter):
        resamples = np.stack([eng.device_multinomial(shots, pvals[t], n_set, out["seed"], first_row=(r * n_iter + t) * n_set)
                              for r in range(n_points)])
        est, info = tmg.point_estimate_batch(resamples, method=method_boot)
        dist = eng.hs_dist(est, rho[t])
        hits[t] = (delta[t] > dist).sum()
    print("delta", delta, "hits", hits, out["hits"])
    assert np.array_equal(out["hits"], hits)
    cls = np.linspace(0, 1, n_points)
    assert np.array_equal(out["levels"], [cls[h - 1] if h else 0.0 for h in hits])
    # the table does not depend on the chunking, and the plain call returns the sorted levels
    again = metrics.get_CL_list_state(state, chunk=2, **kw)
    assert np.array_equal(again["hits"], hits) and np.array_equal(again["counts"], out["counts"])
    kw.pop("return_details")
    assert np.array_equal(metrics.get_CL_list_state(state, chunk=1, **kw), np.sort(out["levels"]))


def _rule(delta, distances, cls):
    """metrics.py:140-144"""
    inside = np.where(delta > distances)[0]
    return 0 if len(inside) == 0 else cls[inside[-1]]


def test_gamma_study_state():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    state = _two_qubit_state()
    n_iter, n_points = 4, 50
    out = metrics.get_CL_list_state(state, n_iter=n_iter, n_points=n_points, interval="gamma", n_measurements=1000, seed=9,
                                    return_details=True)
    cls = np.linspace(0, 1, n_points)
    tmg = qp.StateTomograph(state)
    tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", 2)
    tmg.results = out["counts"][-1]
    radii = qp.MomentInterval(tmg).radii_batch(out["counts"], cls)
    rho, _ = tmg.point_estimate_batch(out["counts"], method="lin")
    delta = tmg._engine().hs_dist(rho, state.matrix)
    assert np.array_equal(out["levels"], [_rule(delta[t], radii[t], cls) for t in range(n_iter)])
    for t in range(n_iter):  # batched against single moments, at the tolerance of tests/test_gpu_moments.py
        t1 = qp.StateTomograph(state)
        t1.povm_matrix, t1.results = tmg.povm_matrix, out["counts"][t]
        assert np.allclose(qp.MomentInterval(t1)(cls)[0], radii[t], rtol=1e-12)
    plain = metrics.get_CL_list_state(state, n_iter=n_iter, n_points=n_points, interval="gamma", n_measurements=1000, seed=9)
    assert np.array_equal(plain, np.sort(out["levels"]))


def test_gamma_study_channel():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    chan = qp.channel.depolarizing(0.1, 1)
    n_iter, n_points = 4, 50
    out = metrics.get_CL_list_channel(chan, n_iter=n_iter, n_points=n_points, interval="gamma", n_measurements=1000, seed=4,
                                      return_details=True)
    cls = np.linspace(0, 1, n_points)
    tmg = qp.ProcessTomograph(chan)
    tmg.experiment_batch(1000, "proj-set")  # (sets the tomographs up; their results are replaced below)
    tmg.results = out["counts"][-1]
    radii = qp.MomentInterval(tmg).radii_batch(out["counts"], cls)
    choi = tmg.point_estimate_batch(out["counts"])
    delta = tmg._engine().hs_dist(choi, chan.choi.matrix)
    assert np.array_equal(out["levels"], [_rule(delta[t], radii[t], cls) for t in range(n_iter)])
    for t in range(n_iter):
        tmg.results = out["counts"][t]
        assert np.allclose(qp.MomentInterval(tmg)(cls)[0], radii[t], rtol=1e-12)


def test_study_smoke():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    state = qp.Qobj(np.array([[0.8, 0.3], [0.3, 0.2]]))
    levels = metrics.get_CL_list_state(state, n_iter=64, n_points=200, interval="boot", n_measurements=1000, seed=1)
    assert levels.shape == (64,) and np.array_equal(levels, np.sort(levels))
    assert levels.min() >= 0 and levels.max() <= 1 and levels.min() < levels.max()
