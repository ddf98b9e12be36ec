"""GPU: the front of the n <= 3 MLE kernels -- the leading plain arguments (counts, image, Ns, B, M, extra, max_iter,
gtol in front of the POVM struct, csrc/qt_args.h: mle_front), which the compiler preloads into SGPRs, and the batch of
loads at the top of a trial that takes its addresses from them.  A mis-ordered or mis-typed argument, or a load that
went ahead of something it needed, shows on the smallest launches: partial
workgroups, a twin wavefront beside dead lanes, a counts pointer that is not the start of its allocation.  Every check is
np.array_equal: a trial's result does not depend on the batch it is launched in, nor on which of the three routes (twin
kernel, k_mle_fused, split pair) runs it.  The counts are those of tests/golden/mle_diet_bits.npz."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROUTES = ("hw", "fused", "split")


@pytest.fixture(scope="module")
def gold():
    return load_golden("mle_diet_bits")


def _engine(n, povm, shots):
    import quantpy_amd as qp

    eng = qp.get_engine(n)
    a = qp.generate_measurement_matrix(povm, n)
    eng.set_povm(a, np.ones(np.asarray(a).shape[0]) * shots)
    return eng


def _run(eng, cd, route, init="lin", max_iter=100, rho=None):
    """One device-pointer call on the counts tensor `cd` (may be a slice) -> dict of host arrays; `rho`: write there."""
    import torch
    from quantpy_amd import _capi

    b, d = cd.shape[0], eng.d
    nit, nfev, status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda")
    if rho is None:
        rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
    try:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1 if route == "hw" else 0)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 0 if route == "split" else 1024)
        eng.mle_dev(cd, rho, init=init, max_iter=max_iter, nit=nit, nfev=nfev, fun=fun, status=status)
        took_hw = eng.mle_helper_wave
        eng.sync()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    assert took_hw == (route == "hw" and init == "lin" and eng.n == 3), (route, init, took_hw)
    return dict(rho=rho.cpu().numpy().view(np.float64), nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(), fun=fun.cpu().numpy(),
                status=status.cpu().numpy())


def _dev(counts):
    import torch

    return torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()


def _take(res, idx):
    return {k: v[idx] for k, v in res.items()}


def _equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


@pytest.fixture(scope="module")
def n3(gold):
    """Twelve 'proj-set' trials (the five of the fixture, repeated), which of them the sweep clips, and the 12-trial
    batch's results through the twin kernel from both starts: the reference of every n = 3 'proj-set' case, computed once."""
    import torch

    counts = gold["n3_ginibre/counts"][np.arange(12) % 5]
    eng = _engine(3, "proj-set", 100000)
    cd = _dev(counts)
    lin = torch.zeros((12, 8, 8), dtype=torch.complex128, device="cuda")
    eng.lin_dev(cd, lin, physical=False)
    eng.sync()
    clipped = np.array([np.linalg.eigvalsh(m).min() < 0 for m in lin.cpu().numpy()])
    assert clipped.any() and not clipped.all(), clipped
    ref = {"lin": _run(eng, cd, "hw"), "mixed": _run(eng, cd, "fused", init="mixed", max_iter=30)}
    assert (ref["lin"]["status"] == 0).all() and (ref["mixed"]["nit"] > 0).all()
    return counts, clipped, ref


def _picks(clipped, b):
    """Index sets of `b` trials each, out of the twelve, that together hold both kinds -- and each set both where b > 1."""
    pd_, cl = np.flatnonzero(~clipped), np.flatnonzero(clipped)
    if b == 1:
        return [pd_[:1], cl[:1]]
    idx = np.concatenate([cl[:1], pd_[:1], np.arange(12)])
    _, first = np.unique(idx, return_index=True)
    return [idx[np.sort(first)][:b]]


@pytest.mark.parametrize("b", [1, 3, 5])
def test_projset_partial_workgroups(n3, b):
    counts, clipped, ref = n3
    eng = _engine(3, "proj-set", 100000)
    picks = _picks(clipped, b)
    kinds = np.concatenate([clipped[p] for p in picks])
    assert kinds.any() and not kinds.all(), (b, kinds)  # a trial the first wave keeps and one its twin takes over
    for p in picks:
        assert len(p) == b
        for route in ROUTES:
            _equal(_run(eng, _dev(counts[p]), route), _take(ref["lin"], p), (b, route, p))


def test_projset_mixed_start(n3):
    """k_mle_fused_mixed and the split pair on iterating trials."""
    counts, clipped, ref = n3
    eng = _engine(3, "proj-set", 100000)
    p = _picks(clipped, 3)[0]
    assert clipped[p].any() and not clipped[p].all()
    for route in ("fused", "split"):
        _equal(_run(eng, _dev(counts[p]), route, init="mixed", max_iter=30), _take(ref["mixed"], p), (route, p))


def test_sic_generic_instantiation(gold):
    counts = gold["n3_sic/counts"]
    eng = _engine(3, "sic", 100000)
    ref = _run(eng, _dev(counts), "hw")
    assert not eng.mle_specialised
    for route in ROUTES:
        _equal(_run(eng, _dev(counts[1:4]), route), _take(ref, slice(1, 4)), route)


@pytest.mark.parametrize("n", [1, 2])
def test_several_trials_per_wave(gold, n):
    counts = gold[f"n{n}_b17/counts"]
    eng = _engine(n, "proj-set", 400)
    ref = _run(eng, _dev(counts[:12]), "fused")
    for route in ("fused", "split"):
        _equal(_run(eng, _dev(counts[3:8]), route), _take(ref, slice(3, 8)), (n, route))


def test_wrong_shots_in_one_setting(n3):
    """Ns is a leading argument: the trial whose counts miss the registered total in ONE setting is flagged, its neighbour
    is not and keeps its result."""
    from quantpy_amd import _capi

    counts, clipped, ref = n3
    eng = _engine(3, "proj-set", 100000)
    two = counts[:2].copy()
    two[1, 13, 0] += 1
    for route in ROUTES:
        got = _run(eng, _dev(two), route)
        assert got["status"][1] == _capi.TRIAL_SHOTS and got["status"][0] == 0, (route, got["status"])
        _equal(_take(got, slice(0, 1)), _take(ref["lin"], slice(0, 1)), route)


def test_pointers_inside_their_allocations(n3):
    """counts_d[7:10] of a 16-trial tensor, and rho written into the middle of a larger tensor."""
    import torch

    counts, clipped, ref = n3
    eng = _engine(3, "proj-set", 100000)
    big = _dev(np.concatenate([counts, counts[:4]]))
    own = {route: _run(eng, _dev(counts[7:10]), route) for route in ROUTES}
    for route in ROUTES:
        _equal(own[route], _take(ref["lin"], slice(7, 10)), route)
        _equal(_run(eng, big[7:10], route), own[route], route)
        rho = torch.full((9, 8, 8), complex(-7.0, 7.0), dtype=torch.complex128, device="cuda")
        got = _run(eng, big[7:10], route, rho=rho[3:6])
        full = rho.cpu().numpy()
        assert (full[:3] == complex(-7.0, 7.0)).all() and (full[6:] == complex(-7.0, 7.0)).all(), route
        assert np.array_equal(full[3:6].view(np.float64), own[route]["rho"]), route
        _equal(got, own[route], route)
