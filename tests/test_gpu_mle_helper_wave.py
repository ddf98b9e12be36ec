"""GPU: the one-launch n = 3 MLE with a helper wavefront per trial (k_mle_fused_hw, QT_OPT_MLE_HELPER_WAVE = 1) against
the same launch without helpers (k_mle_fused, option 0) on one engine.  The helper runs a clipped trial's second
Cholesky sweep beside the front of its first evaluation; no floating-point operation or its order changes, so "equal"
below is np.array_equal: the same bits.  Every call is a device-pointer call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFFSET = 10  # first trial taken from the benchmark's stream: trials 10 .. 18 hold both classes (checked in _classes)


def _ginibre(rng, d, rank=None):
    g = rng.standard_normal((d, rank or d)) + 1j * rng.standard_normal((d, rank or d))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _negatives(oracle, povm, counts):
    """Negative eigenvalues of every trial's unprojected linear-inversion estimate."""
    return np.array([(np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)) < 0).sum() for c in counts])


@pytest.fixture(scope="module")
def data(oracle):
    """The benchmark's recipe (Ginibre state of seed 1234, 1e5 shots per setting, np.random.seed(7)): trials
    OFFSET .. OFFSET + 8 of its stream; and four trials of a rank-1 state at 1e3 shots.  With their classes."""
    povm = oracle.measurement_matrix("proj-set", 3)
    bloch = oracle.bloch_from_matrix(_ginibre(np.random.default_rng(1234), 8))
    np.random.seed(7)
    stream = np.stack([oracle.sample_counts(povm, bloch, np.ones(27) * 100000) for _ in range(OFFSET + 9)])
    head = stream[OFFSET:].astype(np.int64)
    pure = _ginibre(np.random.default_rng(77), 8, rank=1)
    np.random.seed(8)
    low = np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(pure), np.ones(27) * 1000)
                    for _ in range(4)]).astype(np.int64)
    return {"head": head, "head_neg": _negatives(oracle, povm, head), "low": low, "low_neg": _negatives(oracle, povm, low)}


@pytest.fixture(scope="module")
def eng():
    import quantpy_amd as qp

    return qp.get_engine(3)


def _set_povm(eng, shots):
    import quantpy_amd as qp

    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * shots)


def _mle(eng, counts, helper, max_iter=100, with_fun=False, dist_centre=None):
    """One launch with the option at `helper`: everything it writes, and whether it was the kernel with helpers."""
    import torch

    from quantpy_amd import _capi

    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
    nit, nfev, status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda") if with_fun else None
    out = {}
    try:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, helper)
        if dist_centre is None:
            rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
            eng.mle_dev(cd, rho, max_iter=max_iter, nit=nit, nfev=nfev, fun=fun, status=status)
            took = eng.mle_helper_wave
            eng.sync()
            out["rho"] = rho.cpu().numpy().view(np.float64)
        else:
            cen = torch.from_numpy(np.ascontiguousarray(dist_centre, dtype=np.complex128)).cuda()
            dist = torch.zeros(b, dtype=torch.float64, device="cuda")
            eng.mle_dist_dev(cd, cen, dist, max_iter=max_iter, rho=None, nit=nit, nfev=nfev, fun=fun, status=status)
            took = eng.mle_helper_wave
            eng.sync()
            out["dist"] = dist.cpu().numpy()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
    out.update(nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(), status=status.cpu().numpy())
    if with_fun:
        out["fun"] = fun.cpu().numpy()
    return out, took


def _same_bits(eng, counts, **kw):
    on, took_on = _mle(eng, counts, 1, **kw)
    off, took_off = _mle(eng, counts, 0, **kw)
    assert took_on and not took_off
    assert on.keys() == off.keys()
    for k in on:
        assert np.array_equal(on[k], off[k]), (k, on[k], off[k])
    assert (on["status"] != -7).all() and (on["nit"] != -7).all() and (on["nfev"] != -7).all()
    return on


def test_classes_of_the_batches(data):
    """The 9-trial batch holds positive-definite and single-negative trials, one workgroup (4 trials) mixes them, and
    the last, partial workgroup holds a single-negative one; the low-rank trials take the eigensolver."""
    neg = data["head_neg"]
    assert (neg == 0).any() and (neg == 1).any(), neg
    groups = [neg[g:g + 4] for g in range(0, 9, 4)]
    assert any((g == 0).any() and (g == 1).any() for g in groups), neg
    assert neg[8] == 1 and neg[2] == 1 and neg[0] == 0, neg  # B = 9: padded block; B = 3, 4, 5: one clipped; B = 1: PD
    assert (data["low_neg"] >= 2).all(), data["low_neg"]


@pytest.mark.parametrize("b", [1, 3, 4, 5, 9])
def test_partial_workgroups(eng, data, b):
    _set_povm(eng, 100000)
    on = _same_bits(eng, data["head"][:b])
    assert (on["status"] == 0).all(), on["status"]


def test_low_rank_trials_take_no_task(eng, data):
    _set_povm(eng, 1000)
    _same_bits(eng, data["low"])


def test_iterating_trials(eng, data):
    _set_povm(eng, 1000)
    on = _same_bits(eng, data["low"], max_iter=100, with_fun=True)
    assert on["nit"].max() > 0, on["nit"]


def test_mixed_classes_with_fun(eng, data):
    """Clipped, positive-definite and low-rank trials side by side in one workgroup, `fun` asked for."""
    _set_povm(eng, 100000)
    counts = np.concatenate([data["head"][:3], data["low"][:2] * 100])  # (1e3-shot counts scaled to the registered 1e5)
    _same_bits(eng, counts, with_fun=True)


def test_distance_entry(eng, data):
    _set_povm(eng, 100000)
    _same_bits(eng, data["head"][:5], dist_centre=_ginibre(np.random.default_rng(5), 8))


@pytest.mark.parametrize("option", ["QT_OPT_MLE_SPECIALISE", "QT_OPT_PAIRED_STAGES"])
def test_generic_instantiation(eng, data, option):
    from quantpy_amd import _capi

    _set_povm(eng, 100000)
    try:
        eng.set_option(getattr(_capi, option), 0)
        _same_bits(eng, data["head"][:5], with_fun=True)
        assert not eng.mle_specialised
    finally:
        eng.set_option(getattr(_capi, option), 1)


def test_option_round_trip(eng, data):
    _set_povm(eng, 100000)
    counts = data["head"][:4]
    took = [_mle(eng, counts, v)[1] for v in (1, 0, 1)]
    assert took == [True, False, True]
    import torch

    cd = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
    rho = torch.zeros((4, 8, 8), dtype=torch.complex128, device="cuda")
    eng.mle_dev(cd, rho, init="mixed")  # the mixed start keeps its own kernel
    assert not eng.mle_helper_wave
    eng.sync()
