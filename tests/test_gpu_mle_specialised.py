"""GPU: the MLE kernels specialised on the launch-uniform shape of a six-projector POVM (template parameter
GENERIC = false: product POVM with R1 = 6, both tables paired, equal shots, segmented shots check) against the generic
instantiation of the same kernels, on one engine (QT_OPT_MLE_SPECIALISE 1 / 0).  The specialisation removes run-time
decisions, spills and table staging and keeps every floating-point operation and its order, so "equal" below is
np.array_equal: the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _ginibre(rng, d, rank=None):
    g = rng.standard_normal((d, rank or d)) + 1j * rng.standard_normal((d, rank or d))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _run(eng, capi, counts, centre):
    """Everything the MLE kernels write, through the device-pointer calls (a trial flagged QT_TRIAL_SHOTS must come
    back as status 5, not as the exception of the NumPy-level calls): both starts through the one-launch form and
    the split pair, the one-pass distance, and 'lin'."""
    import torch

    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    cen = torch.from_numpy(np.ascontiguousarray(centre, dtype=np.complex128)).cuda()
    out, spec = {}, {}

    def new(dtype, *shape):
        return torch.zeros(shape, dtype=dtype, device="cuda")

    try:
        for path, waves in (("fused", 1024), ("split", 0)):
            eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
            for init in ("lin", "mixed"):
                rho, fun = new(torch.complex128, b, d, d), new(torch.float64, b)
                nit, nfev, status = (new(torch.int32, b) for _ in range(3))
                eng.mle_dev(cd, rho, init=init, nit=nit, nfev=nfev, fun=fun, status=status)
                spec[f"{path}_{init}"] = eng.mle_specialised
                dist, st2 = new(torch.float64, b), new(torch.int32, b)
                eng.mle_dist_dev(cd, cen, dist, init=init, status=st2)
                spec[f"{path}_{init}_dist"] = eng.mle_specialised
                eng.sync()
                for k, v in (("rho", rho), ("nit", nit), ("nfev", nfev), ("fun", fun), ("status", status), ("dist", dist),
                             ("dist_status", st2)):
                    a = v.cpu().numpy()
                    out[f"{path}_{init}_{k}"] = a.view(np.float64) if a.dtype == np.complex128 else a
    finally:
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    rho, status = new(torch.complex128, b, d, d), new(torch.int32, b)
    eng.lin_dev(cd, rho, status=status)
    eng.sync()
    out["lin_rho"], out["lin_status"] = rho.cpu().numpy().view(np.float64), status.cpu().numpy()
    return out, spec


def _on_off(eng, capi, counts, centre):
    try:
        eng.set_option(capi.QT_OPT_MLE_SPECIALISE, 1)
        on, spec_on = _run(eng, capi, counts, centre)
        eng.set_option(capi.QT_OPT_MLE_SPECIALISE, 0)
        off, spec_off = _run(eng, capi, counts, centre)
    finally:
        eng.set_option(capi.QT_OPT_MLE_SPECIALISE, 1)
    assert not any(spec_off.values()), spec_off
    return on, off, spec_on


def _assert_same_bits(on, off, what):
    assert on.keys() == off.keys()
    for k in on:
        assert np.array_equal(on[k], off[k]), (what, k)


def _headline_batch(oracle):
    """13 trials at n = 3: 10 from the first 64 of the benchmark's stream (at least 3 positive definite linear
    inversions, at least 3 with exactly one negative eigenvalue), 2 of a rank-1 state at 100 shots per setting (two or
    more negative eigenvalues: the eigensolver fallback) and 1 with one setting's counts doubled (status 5).  13 leaves
    the last workgroup with one live wave and three padding waves."""
    povm = oracle.measurement_matrix("proj-set", 3)
    bloch = oracle.bloch_from_matrix(_ginibre(np.random.default_rng(1234), 8))
    np.random.seed(7)
    stream = np.stack([oracle.sample_counts(povm, bloch, np.ones(27) * 100000) for _ in range(64)])
    neg = np.array([(np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)) < 0).sum() for c in stream])
    pd_, one = np.flatnonzero(neg == 0), np.flatnonzero(neg == 1)
    assert pd_.size >= 3 and one.size >= 3, (pd_.size, one.size)
    n_pd = min(pd_.size, 10 - min(one.size, 5))
    pick = np.concatenate([pd_[:n_pd], one[:10 - n_pd]])
    assert pick.size == 10 and n_pd >= 3 and 10 - n_pd >= 3
    pure = _ginibre(np.random.default_rng(77), 8, rank=1)
    np.random.seed(8)
    low = np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(pure), np.ones(27) * 100) for _ in range(2)])
    for c in low:
        assert (np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)) < 0).sum() >= 2
    # (equal shots per setting: the totals of a 100-shot trial are proportional to the registered 1e5, the check passes)
    bad = stream[int(pick[0])].copy()
    bad[5] *= 2
    return np.concatenate([stream[pick], low, bad[None]]).astype(np.int64), len(pick) + len(low)


def test_n3_specialised_kernels_give_the_bits_of_the_generic_ones(qp, oracle):
    from quantpy_amd import _capi

    counts, i_bad = _headline_batch(oracle)
    assert counts.shape == (13, 27, 8)
    eng = qp.get_engine(3)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * 100000)
    centre = _ginibre(np.random.default_rng(5), 8)
    on, off, spec = _on_off(eng, _capi, counts, centre)
    assert all(spec.values()), spec
    _assert_same_bits(on, off, "n3")
    for path in ("fused", "split"):
        for init in ("lin", "mixed"):
            st = on[f"{path}_{init}_status"]
            assert st[i_bad] == 5 and (np.delete(st, i_bad) != 5).all(), (path, init, st)
            assert on[f"{path}_{init}_dist_status"][i_bad] == 5
            if init == "mixed":  # every trial with good shots iterates
                assert (np.delete(on[f"{path}_{init}_nit"], i_bad) > 0).all()
    assert on["lin_status"][i_bad] == 5


@pytest.mark.parametrize("n,b", [(2, 21), (1, 70)])
def test_small_n_partial_waves_and_workgroups(qp, oracle, n, b):
    """n = 2: 4 trials per wave, 21 trials = one full workgroup and a second with one full wave and a quarter of one;
    n = 1: 16 trials per wave, 70 trials = one full workgroup and six lanes' worth of a fifth wave."""
    from quantpy_amd import _capi

    d = 2**n
    rng = np.random.default_rng(40 + n)
    povm = oracle.measurement_matrix("proj-set", n)
    np.random.seed(50 + n)
    states = [_ginibre(rng, d), _ginibre(rng, d, rank=1)]
    counts = np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(states[t % 2]), np.ones(3**n) * 400)
                       for t in range(b)])
    eng = qp.get_engine(n)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * 400)
    on, off, spec = _on_off(eng, _capi, counts, states[0])
    assert all(spec.values()), spec
    _assert_same_bits(on, off, n)
    assert (on["fused_mixed_nit"] > 0).all() and (on["fused_lin_status"] != 5).all()


@pytest.mark.parametrize("case", ["sic", "unequal-shots", "plain-array", "paired-stages-off"])
def test_ineligible_povms_take_the_generic_kernels(qp, oracle, case):
    from quantpy_amd import _capi

    n, d = 2, 4
    rng = np.random.default_rng(60)
    name = "sic" if case == "sic" else "proj-set"
    a_prod = qp.generate_measurement_matrix(name, n)
    a_dense = np.array(a_prod)
    s = a_dense.shape[0]
    shots = np.array([300 + 50 * (k % 3) for k in range(s)], dtype=float) if case == "unequal-shots" else np.ones(s) * 400
    np.random.seed(61)
    rho = _ginibre(rng, d)
    counts = np.stack([oracle.sample_counts(a_dense, oracle.bloch_from_matrix(rho), shots) for _ in range(9)])
    eng = qp.get_engine(n)
    eng.set_povm(a_dense if case == "plain-array" else a_prod, shots)
    try:
        if case == "paired-stages-off":
            eng.set_option(_capi.QT_OPT_PAIRED_STAGES, 0)
        on, off, spec = _on_off(eng, _capi, counts, rho)
    finally:
        eng.set_option(_capi.QT_OPT_PAIRED_STAGES, 1)
    assert not any(spec.values()), spec
    _assert_same_bits(on, off, case)
