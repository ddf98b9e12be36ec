"""GPU: the bootstrap coverage study for processes (quantpy_amd.metrics.get_CL_list_channel_boot, reference
metrics.py:282-316) and what it is made of.

* qt_lifp_dist_group_batch measures process b of a resample-major batch against centre b % G.  The arithmetic is that of
  qt_lifp_dist_batch and only the centre's address differs, so `dist`, `iters` and `status` are compared BIT FOR BIT with
  G ungrouped calls on counts[g::G] with centre g -- on the default paths, whose kernels do not depend on the batch size.
  On the dense-operator paths of n = 2 (chosen from the batch size) the whole batch is compared with qt_lifp_batch plus
  qt_hs_dist_dim per group: bit for bit where k_hs_dist forms the distance, and within 1e-15 + D^2 2^-53 dist -- the
  re-ordering bound derived in tests/test_gpu_process_bootstrap_fused.py -- where k_cptp_wave16 does.
* qt_process_born_probs against Channel.transform and the host Born rule, within 1e-13 absolute: a probability is a sum
  of at most 4^n = 64 products of magnitude <= 1 formed twice (channel, then Born rule), i.e. a few hundred roundings of
  2^-53 ~ 1.1e-16 at the very worst ~ 3e-14.
* the study against the documented keying, redrawn resample by resample with the ungrouped sampler and estimator."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BMAX = {1: 37, 2: 3077, 3: 5}
SHOTS = 1000


@functools.lru_cache(maxsize=None)
def _tomograph(n):
    """depolarizing(0.1, n) probed with 'proj4' inputs and 'proj-set' at 1000 shots, and BMAX[n] experiments of it."""
    import quantpy_amd as qp

    np.random.seed(60 + n)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, n), input_states="proj4")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=BMAX[n])
    counts.setflags(write=False)
    return tmg, counts


def _engine(n):
    """The cached engine of this size with the fixture's POVM, shots and input states (other tests register their own)."""
    return _tomograph(n)[0]._engine()


def _lifp(eng, counts, cptp):
    """qt_lifp_batch on device pointers: (choi, iters, status)."""
    import torch

    b, dd = counts.shape[:2]
    choi = torch.zeros((b, dd, dd), dtype=torch.complex128, device="cuda")
    iters = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    status = torch.full((b,), -1, dtype=torch.int32, device="cuda")
    eng.lifp_dev(torch.from_numpy(np.array(counts)).cuda(), choi, cptp=cptp, iters=iters, status=status)
    eng.sync()
    return choi.cpu().numpy(), iters.cpu().numpy(), status.cpu().numpy()


def _dist_dev(eng, counts, centre, cptp, with_choi=True):
    """qt_lifp_dist_batch / qt_lifp_dist_group_batch on device pointers: (dist, choi or None, iters, status).  Three
    guard elements behind row B must stay as they were."""
    import torch

    b, dd = counts.shape[:2]
    cd = torch.from_numpy(np.array(counts)).cuda()
    cen = torch.from_numpy(np.array(centre, dtype=np.complex128)).cuda()
    dist = torch.full((b + 3,), -7.0, dtype=torch.float64, device="cuda")
    iters = torch.full((b + 3,), -7, dtype=torch.int32, device="cuda")
    status = torch.full((b + 3,), -7, dtype=torch.int32, device="cuda")
    choi = torch.zeros((b, dd, dd), dtype=torch.complex128, device="cuda") if with_choi else None
    eng.lifp_dist_dev(cd, cen, dist[:b], cptp=cptp, choi=choi, iters=iters[:b], status=status[:b])
    eng.sync()
    dist, iters, status = dist.cpu().numpy(), iters.cpu().numpy(), status.cpu().numpy()
    assert (dist[b:] == -7.0).all() and (iters[b:] == -7).all() and (status[b:] == -7).all()
    return dist[:b], None if choi is None else choi.cpu().numpy(), iters[:b], status[:b]


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@functools.lru_cache(maxsize=None)
def _estimates(n, cptp):
    """(choi, iters, status) of qt_lifp_batch on all BMAX[n] experiments, default paths, computed once."""
    out = _lifp(_engine(n), _tomograph(n)[1], cptp)
    for a in out:
        a.setflags(write=False)
    return out


GROUPED = [(1, 37, 5, True), (1, 37, 5, False), (2, 37, 5, True), (2, 37, 5, False), (2, 3077, 7, False), (3, 5, 3, True),
           (3, 5, 3, False)]


@pytest.mark.parametrize("n,b,g,cptp", GROUPED)
def test_grouped_equals_ungrouped(n, b, g, cptp):
    """Default paths: every group of the grouped call carries the bits of the ungrouped call on that group's processes
    with that group's centre; iters and status too; with and without `choi`, which is qt_lifp_batch's; the first G
    distances (each centre against itself) are exactly 0.  B = 3077 without the projection sends k_lifp16's stride loop
    round a second time; B = 37 with G = 5 leaves a partial last group and a partial last workgroup."""
    eng = _engine(n)
    counts = _tomograph(n)[1][:b]
    choi2, iters2, status2 = (a[:b] for a in _estimates(n, cptp))
    centres = choi2[:g]
    host, info = eng.lifp_dist(counts, centres, cptp=cptp, return_info=True)
    for k in range(g):
        one, info1 = eng.lifp_dist(counts[k::g], centres[k], cptp=cptp, return_info=True)
        assert _same_bits(host[k::g], one), (k, host[k::g], one)
        assert np.array_equal(info["iters"][k::g], info1["iters"]) and np.array_equal(info["status"][k::g], info1["status"])
    assert np.all(host[:g] == 0.0) and np.all(host[g:] > 0) and np.isfinite(host).all()
    assert np.array_equal(info["iters"], iters2) and np.array_equal(info["status"], status2)
    # a wrong centre shows: group 0 against centre 1 gives other distances
    assert not np.array_equal(eng.lifp_dist(counts[0::g], centres[1], cptp=cptp), host[0::g])
    for with_choi in (True, False):
        dist, choi, iters, status = _dist_dev(eng, counts, centres, cptp, with_choi)
        assert _same_bits(dist, host) and np.array_equal(iters, iters2) and np.array_equal(status, status2)
        if with_choi:
            assert np.array_equal(choi, choi2)


@pytest.mark.parametrize("b", [37, 300])
@pytest.mark.parametrize("cptp", [True, False])
def test_dense_operator_paths(b, cptp):
    """n = 2 on the dense left inverse, G = 5, the whole batch: k_lifp_batch<16> (B = 37) and k_lifp_gemm (B = 300) store
    their matrices and k_hs_dist reads them -- the bits of qt_lifp_batch + qt_hs_dist_dim per group -- except where
    k_cptp_wave16 projects after the GEMM and forms the distance itself, in another order of the 256 terms."""
    g = 5
    eng = _engine(2)
    counts = _tomograph(2)[1][:b]
    eng.process_prefer_dense(True)
    try:
        choi2, _, _ = _lifp(eng, counts, cptp)
        centres = choi2[:g].copy()
        dist, choi, _, status = _dist_dev(eng, counts, centres, cptp)
        none, _, _, _ = _dist_dev(eng, counts, centres, cptp, with_choi=False)
    finally:
        eng.process_prefer_dense(False)
    two = np.empty(b)
    for k in range(g):
        two[k::g] = eng.hs_dist(choi2[k::g], centres[k])
    print(f"B={b} cptp={cptp}: max |grouped - two-pass| = {np.abs(dist - two).max():.3e}, max two-pass = {two.max():.3e}")
    assert np.array_equal(choi, choi2) and not status.any() and _same_bits(none, dist) and np.all(dist[:g] == 0.0)
    if cptp and b == 300:
        assert np.all(np.abs(dist - two) <= 1e-15 + 256.0 * 2.0**-53 * np.abs(two)), np.abs(dist - two).max()
    else:
        assert _same_bits(dist, two)


@pytest.mark.parametrize("n,b,g,slice_,cptp", [(3, 5, 3, 2, True), (3, 5, 3, 2, False), (2, 37, 3, 5, True), (2, 37, 3, 5, False)])
def test_slices_carry_the_group(n, b, g, slice_, cptp):
    """A slice that starts at b0 starts in group b0 % G: slices whose length is no multiple of G give the unsliced bits,
    with the matrices in the handle's workspace (n = 3) and with the distance formed in the kernels (n = 2)."""
    from quantpy_amd import _capi

    eng = _engine(n)
    counts = _tomograph(n)[1][:b]
    centres = _estimates(n, cptp)[0][:g]
    whole, info_w = eng.lifp_dist(counts, centres, cptp=cptp, return_info=True)
    eng.set_option(_capi.QT_OPT_LIFP_DIST_SLICE, slice_)
    try:
        sliced, info_s = eng.lifp_dist(counts, centres, cptp=cptp, return_info=True)
        dev, choi, _, _ = _dist_dev(eng, counts, centres, cptp)
    finally:
        eng.set_option(_capi.QT_OPT_LIFP_DIST_SLICE, 0)
    assert _same_bits(sliced, whole) and _same_bits(dev, whole) and np.array_equal(choi, _estimates(n, cptp)[0][:b])
    assert np.array_equal(info_s["iters"], info_w["iters"]) and np.array_equal(info_s["status"], info_w["status"])
    assert np.all(whole[:g] == 0.0) and np.all(whole[g:] > 0)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("cptp", [True, False])
def test_one_group_is_the_old_entry(n, cptp):
    eng = _engine(n)
    b = min(BMAX[n], 37)
    counts = _tomograph(n)[1][:b]
    centre = _estimates(n, cptp)[0][0]
    old, info_o = eng.lifp_dist(counts, centre, cptp=cptp, return_info=True)
    new, info_n = eng.lifp_dist(counts, centre[None], cptp=cptp, return_info=True)
    assert _same_bits(new, old) and new[0] == 0.0
    assert np.array_equal(info_n["iters"], info_o["iters"]) and np.array_equal(info_n["status"], info_o["status"])


def test_argument_checks():
    """G = 0 is QT_ERR_ARG and writes nothing; the host-pointer and the device-pointer call give the same bits (n = 2)."""
    import quantpy_amd.engine as qe
    from quantpy_amd import _capi

    eng = _engine(1)
    c = np.ascontiguousarray(_tomograph(1)[1][:4])
    centres = np.ascontiguousarray(_estimates(1, True)[0][:2])
    dist, iters, status = np.full(4, -7.0), np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
    call = eng.lib.qt_lifp_dist_group_batch
    for g in (0, -1):
        assert call(eng._h, c.ctypes.data, 4, 1, centres.ctypes.data, g, None, dist.ctypes.data, iters.ctypes.data,
                    status.ctypes.data, _capi.QT_HOST_PTR) == _capi.QT_ERR_ARG
    assert call(eng._h, c.ctypes.data, 4, 1, None, 2, None, dist.ctypes.data, None, None, _capi.QT_HOST_PTR) == _capi.QT_ERR_ARG
    assert np.all(dist == -7.0) and np.all(iters == -7) and np.all(status == -7)
    with pytest.raises(qe.EngineError):
        eng.lifp_dist(c, centres[:0])
    assert call(eng._h, c.ctypes.data, 4, 1, centres.ctypes.data, 2, None, dist.ctypes.data, iters.ctypes.data,
                status.ctypes.data, _capi.QT_HOST_PTR) == 0
    assert np.all(dist[:2] == 0.0) and np.all(dist[2:] > 0) and not status.any()
    fresh = qe.Engine(1)
    try:
        assert fresh.lib.qt_lifp_dist_group_batch(fresh._h, c.ctypes.data, 4, 1, centres.ctypes.data, 2, None, dist.ctypes.data,
                                                  None, None, _capi.QT_HOST_PTR) == _capi.QT_ERR_STATE
        p = np.empty((2, 4, 3, 2))
        # no POVM on this handle: need_povm's code
        assert fresh.lib.qt_process_born_probs(fresh._h, centres.ctypes.data, 2, p.ctypes.data,
                                               _capi.QT_HOST_PTR) == _capi.QT_ERR_STATE
    finally:
        fresh.close()
    eng2 = _engine(2)
    counts2, centres2 = _tomograph(2)[1][:37], _estimates(2, True)[0][:5]
    for cptp in (True, False):
        host, info = eng2.lifp_dist(counts2, centres2, cptp=cptp, return_info=True)
        dev, _, iters_d, status_d = _dist_dev(eng2, counts2, centres2, cptp, with_choi=False)
        assert _same_bits(host, dev) and np.array_equal(info["iters"], iters_d) and np.array_equal(info["status"], status_d)


def test_process_born_probs_argument_checks():
    """Null `choi` or `p` and a negative G are QT_ERR_ARG, G = 0 is a successful call that writes nothing, and a handle
    with a POVM but without qt_process_setup is QT_ERR_STATE."""
    import quantpy_amd as qp
    import quantpy_amd.engine as qe
    from quantpy_amd import _capi

    eng = _engine(1)
    choi = np.ascontiguousarray(_estimates(1, True)[0][:2])
    p = np.full((2, 4, eng.S, eng.K), -7.0)
    call = eng.lib.qt_process_born_probs
    assert call(eng._h, None, 2, p.ctypes.data, _capi.QT_HOST_PTR) == _capi.QT_ERR_ARG
    assert call(eng._h, choi.ctypes.data, 2, None, _capi.QT_HOST_PTR) == _capi.QT_ERR_ARG
    assert call(eng._h, choi.ctypes.data, -1, p.ctypes.data, _capi.QT_HOST_PTR) == _capi.QT_ERR_ARG
    assert call(eng._h, choi.ctypes.data, 0, p.ctypes.data, _capi.QT_HOST_PTR) == 0
    assert call(eng._h, None, 0, None, _capi.QT_HOST_PTR) == 0
    assert np.all(p == -7.0)
    assert eng.process_born_probs(choi[:0]).shape == (0, 4, eng.S, eng.K)
    fresh = qe.Engine(1)
    try:
        fresh.set_povm(qp.generate_measurement_matrix("proj-set", 1), np.full(3, SHOTS))
        assert fresh.lib.qt_process_born_probs(fresh._h, choi.ctypes.data, 2, p.ctypes.data,
                                               _capi.QT_HOST_PTR) == _capi.QT_ERR_STATE
    finally:
        fresh.close()
    assert np.all(p == -7.0)
    assert call(eng._h, choi.ctypes.data, 2, p.ctypes.data, _capi.QT_HOST_PTR) == 0
    assert p.min() >= 0.0 and p.max() <= 1.0 and np.abs(p.sum(-1) - 1.0).max() <= 1e-10


@pytest.mark.parametrize("n", [1, 2, 3])
def test_process_born_probs(n):
    """The true channel, a CPTP-projected estimate and a raw 10-shot estimate (negative probabilities before the clip)
    against np.clip(born_probabilities(povm, Channel(C).transform(rho_i).bloch), 0, 1)."""
    import torch

    import quantpy_amd as qp
    from quantpy_amd.tomography.state import born_probabilities

    tmg, counts = _tomograph(n)
    povm = np.asarray(tmg.tomographs[0].povm_matrix)
    d = 2**n

    def host(c):
        """(the reference table, the smallest probability before the clip) of the channel with Choi matrix c"""
        ch = qp.Channel(qp.Qobj(c))
        blochs = [ch.transform(rho).bloch for rho in tmg.input_basis.elements]
        lowest = min((np.einsum("ijk,k->ij", povm, bl) * d).min() for bl in blochs)
        return np.array([np.clip(born_probabilities(povm, bl), 0, 1) for bl in blochs]), lowest

    # Four 10-shot experiments, unprojected; the one whose host probabilities reach furthest below 0 is the third case.
    # (At n = 1 the inversion is exactly determined and reproduces the observed frequencies, zeros included, up to
    # rounding: the negative entries there are of the order of 1e-17.  At n = 2, 3 they are of the order of 0.1.)
    np.random.seed(70 + n)
    low = qp.ProcessTomograph(tmg.channel, input_states="proj4")
    raws = low.point_estimate_batch(low.experiment_batch(10, "proj-set", repeats=4), cptp=False)
    eng = _engine(n)  # back to the fixture's shots
    candidates = [host(c) for c in raws]
    pick = int(np.argmin([lowest for _, lowest in candidates]))
    chois = np.stack([np.asarray(tmg.channel.choi.matrix, dtype=np.complex128), _estimates(n, True)[0][0], raws[pick]])
    tables = [host(chois[0]), host(chois[1]), candidates[pick]]
    want = np.stack([t[0] for t in tables])
    unclipped_min = np.array([t[1] for t in tables])
    assert unclipped_min[2] < 0 and (want[2] == 0.0).any(), unclipped_min  # at least one entry of the raw estimate is clipped
    got = eng.process_born_probs(chois)
    print(f"n={n}: max |p - reference| = {np.abs(got - want).max():.3e}, unclipped minima {unclipped_min}")
    assert got.shape == want.shape and got.min() >= 0.0 and got.max() <= 1.0
    assert np.abs(got - want).max() <= 1e-13
    assert np.abs(got[:2].sum(-1) - 1.0).max() <= 1e-10
    dev = eng.process_born_probs(torch.from_numpy(chois).cuda())
    out = torch.full((3 * 4**n * povm.shape[0] * povm.shape[1] + 3,), -7.0, dtype=torch.float64, device="cuda")
    eng.process_born_probs(torch.from_numpy(chois).cuda(), out=out[:-3])
    eng.sync()
    assert _same_bits(dev.cpu().numpy(), got) and _same_bits(out[:-3].cpu().numpy().reshape(got.shape), got)
    assert (out[-3:].cpu().numpy() == -7.0).all()


@pytest.mark.parametrize("n,n_iter,n_points", [(1, 3, 5), (2, 2, 3)])
@pytest.mark.parametrize("cptp", [True, False])
def test_study_from_the_documented_keys(n, n_iter, n_points, cptp):
    import quantpy_amd as qp
    from quantpy_amd import metrics

    channel = qp.channel.depolarizing(0.1, n)
    seed = 1234 + n
    kw = dict(n_iter=n_iter, n_points=n_points, n_measurements=SHOTS, cptp=cptp, seed=seed)
    out = metrics.get_CL_list_channel_boot(channel, return_details=True, **kw)
    assert out["seed"] == seed + 1
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=n_iter, sampler="device", seed=seed)
    assert np.array_equal(out["counts"], counts)
    estimates = tmg.point_estimate_batch(counts, method="lifp")
    eng = tmg._engine()
    assert np.array_equal(out["estimates"], estimates)
    assert _same_bits(out["delta"], eng.hs_dist(estimates, channel.choi.matrix))
    dd, s, k = eng.D, eng.S, eng.K
    pvals = eng.process_born_probs(out["estimates"])
    shots = np.tile(np.full(s, SHOTS, dtype=np.int64), dd)
    hits = np.zeros(n_iter, dtype=np.int64)
    for t in range(n_iter):
        resamples = np.stack([eng.device_multinomial(shots, pvals[t].reshape(dd * s, k), dd * s, seed + 1,
                                                     first_row=(r * n_iter + t) * dd * s).reshape(dd, s, k)
                              for r in range(n_points)])
        assert (resamples.sum(-1) == SHOTS).all()
        dist = eng.lifp_dist(resamples, estimates[t], cptp=cptp)
        hits[t] = (out["delta"][t] > dist).sum()
    assert np.array_equal(out["hits"], hits), (out["hits"], hits)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    for chunk in (1, 2):
        again = metrics.get_CL_list_channel_boot(channel, return_details=True, chunk=chunk, **kw)
        assert np.array_equal(again["hits"], hits) and np.array_equal(again["counts"], counts)
    assert np.array_equal(metrics.get_CL_list_channel_boot(channel, **kw), np.sort(out["levels"]))


def test_study_smoke():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    levels = metrics.get_CL_list_channel_boot(qp.channel.depolarizing(0.1, 1), n_iter=64, n_points=200, seed=5)
    assert levels.shape == (64,) and np.array_equal(levels, np.sort(levels))
    assert levels.min() >= 0.0 and levels.max() <= 1.0 and levels.min() < levels.max()
