"""GPU: the likelihood value of an MLE trial's first evaluation is formed only where something reads it (the caller's
`fun`, the hand-off to BFGS, the NaN term of status 4) in the kernels specialised on the six-projector shape; the
generic kernels form it always.  Nothing that reaches an output changes, so every comparison below is np.array_equal.
Inputs as in test_gpu_mle_specialised.py (oracle stream, seeds in this file); every call is a device-pointer call, so
that a trial with bad shots comes back as status 5."""
import numpy as np
import pytest

from test_gpu_mle_specialised import _ginibre, _headline_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _mle(eng, counts, init, want_fun, max_iter=100, centre=None):
    """One mle_dev call (and one mle_dist_dev call without `fun` if `centre` is given) -> dict of host arrays."""
    import torch

    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
    nit, nfev, status = (torch.zeros(b, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda") if want_fun else None
    eng.mle_dev(cd, rho, init=init, max_iter=max_iter, nit=nit, nfev=nfev, fun=fun, status=status)
    out = {"spec": eng.mle_specialised}
    if centre is not None:
        cen = torch.from_numpy(np.ascontiguousarray(centre, dtype=np.complex128)).cuda()
        dist = torch.zeros(b, dtype=torch.float64, device="cuda")
        eng.mle_dist_dev(cd, cen, dist, init=init, max_iter=max_iter)
        eng.sync()
        out["dist"] = dist.cpu().numpy()
    eng.sync()
    out.update(rho=rho.cpu().numpy().view(np.float64), nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(),
               status=status.cpu().numpy())
    if want_fun:
        out["fun"] = fun.cpu().numpy()
    return out


def _dist_with_everything(eng, counts, centre, init):
    """mle_dist_dev with every output asked for, `fun` included: (dist, rho)."""
    import torch

    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    cen = torch.from_numpy(np.ascontiguousarray(centre, dtype=np.complex128)).cuda()
    dist, fun = (torch.zeros(b, dtype=torch.float64, device="cuda") for _ in range(2))
    rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
    nit, nfev, st = (torch.zeros(b, dtype=torch.int32, device="cuda") for _ in range(3))
    eng.mle_dist_dev(cd, cen, dist, init=init, rho=rho, nit=nit, nfev=nfev, fun=fun, status=st)
    eng.sync()
    return dist.cpu().numpy(), rho.cpu().numpy().view(np.float64)


def _check_with_and_without_fun(eng, capi, counts, centre, want_spec=True):
    try:
        for waves in (1024, 0):
            eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
            for init in ("lin", "mixed"):
                a = _mle(eng, counts, init, True, centre=centre)
                b = _mle(eng, counts, init, False, centre=centre)
                assert a["spec"] == want_spec and b["spec"] == want_spec
                for k in ("rho", "nit", "nfev", "status", "dist"):
                    assert np.array_equal(a[k], b[k], equal_nan=True), (waves, init, k)
                ref_dist, ref_rho = _dist_with_everything(eng, counts, centre, init)
                assert np.array_equal(b["dist"], ref_dist, equal_nan=True), (waves, init)
                assert np.array_equal(b["rho"], ref_rho, equal_nan=True), (waves, init)
                # the distance belongs to the rho of the same launch form: recomputed on the host it agrees to rounding
                good = b["status"] == 0
                r = b["rho"].view(np.complex128)[good] - centre
                host = np.sqrt(np.abs(np.einsum("bij,bji->b", r, r))) / np.sqrt(2.0)
                assert np.abs(b["dist"][good] - host).max() < 1e-12
    finally:
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)


def test_n3_same_outputs_with_and_without_fun(qp, oracle):
    from quantpy_amd import _capi

    counts, i_bad = _headline_batch(oracle)
    assert counts.shape == (13, 27, 8)
    eng = qp.get_engine(3)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * 100000)
    centre = _ginibre(np.random.default_rng(5), 8)
    _check_with_and_without_fun(eng, _capi, counts, centre)
    # max_iter = 0: nothing iterates, the good trials report status 3 whether the value is formed or not
    try:
        for waves in (1024, 0):
            eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
            a = _mle(eng, counts, "lin", True, max_iter=0)
            b = _mle(eng, counts, "lin", False, max_iter=0)
            for k in ("rho", "nit", "nfev", "status"):
                assert np.array_equal(a[k], b[k]), (waves, k)
            assert b["status"][i_bad] == 5 and (np.delete(b["status"], i_bad) == 3).all(), b["status"]
            assert (b["nit"] == 0).all()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)


@pytest.mark.parametrize("n,b", [(2, 21), (1, 70)])
def test_small_n_same_outputs_with_and_without_fun(qp, oracle, n, b):
    """Several trials per wave and a partial last wave (the batches of test_small_n_partial_waves_and_workgroups)."""
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
    _check_with_and_without_fun(eng, _capi, counts, states[0])


@pytest.mark.parametrize("n,b,shots,seed", [(1, 20, 400, 70), (2, 6, 10000, 72)])
def test_wave_with_groups_that_need_the_value_and_groups_that_do_not(qp, oracle, n, b, shots, seed):
    """'lin' start, trials of the FIRST wave (16 at n = 1, 4 at n = 2) of which some stop at iteration 0 and some
    iterate (asserted through the oracle): the wave forms the value for the groups that go on, the others must not be
    disturbed by it, and without `fun` nothing changes."""
    from quantpy_amd import _capi

    d, tpw = 2**n, 64 // 4**n
    rng = np.random.default_rng(40 + n)
    povm = oracle.measurement_matrix("proj-set", n)
    states = [_ginibre(rng, d), _ginibre(rng, d, rank=1)]
    np.random.seed(seed)
    counts = np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(states[t % 2]), np.ones(3**n) * shots)
                       for t in range(b)])
    ref_nit = np.array([oracle.mle_estimate(c, povm, return_info=True, solver="port")[1]["nit"] for c in counts])
    assert (ref_nit[:tpw] == 0).any() and (ref_nit[:tpw] > 0).any(), ref_nit
    eng = qp.get_engine(n)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * shots)
    try:
        for waves in (1024, 0):
            eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
            a = _mle(eng, counts, "lin", True)
            o = _mle(eng, counts, "lin", False)
            assert a["spec"] and o["spec"]
            for k in ("rho", "nit", "status"):
                assert np.array_equal(a[k], o[k]), (waves, k)
            assert np.array_equal(o["nit"], ref_nit), (waves, o["nit"], ref_nit)
            assert (o["status"] == 0).all()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)


@pytest.mark.parametrize("shots_check", [0, 1])
def test_n3_all_zero_counts_are_routed_as_a_nan_not_a_fault(qp, oracle, shots_check):
    """One trial of a good batch has all counts zero: its frequencies are 0 / 0.  With the shots check off
    (`shots_check` = 0, the case the NaN tests of status 4 exist for; the engine then takes the generic kernels whatever
    QT_OPT_MLE_SPECIALISE says) and on (the specialised kernels: every p of that trial is a NaN, so the deferred value is
    formed after all) the trial's status is non-zero, the same with and without `fun` and in both instantiations, and
    the other trials do not notice."""
    from quantpy_amd import _capi

    counts, i_bad = _headline_batch(oracle)
    counts = np.delete(counts, i_bad, axis=0)  # an otherwise good batch
    zeroed = counts.copy()
    i_zero = 4
    zeroed[i_zero] = 0
    eng = qp.get_engine(3)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * 100000)
    runs = {}
    try:
        eng.set_option(_capi.QT_OPT_SHOTS_CHECK, shots_check)
        for spec in (1, 0):
            eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, spec)
            for waves in (1024, 0):
                eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
                for init in ("lin", "mixed"):
                    clean = _mle(eng, counts, init, True)
                    for want_fun in (True, False):
                        r = runs[spec, waves, init, want_fun] = _mle(eng, zeroed, init, want_fun)
                        assert r["spec"] == bool(spec and shots_check)
                        assert r["status"][i_zero] != 0, (spec, waves, init, want_fun, r["status"])
                        for k in ("rho", "nit", "nfev", "status") + (("fun",) if want_fun else ()):
                            assert np.array_equal(np.delete(r[k], i_zero, axis=0), np.delete(clean[k], i_zero, axis=0)), \
                                (spec, waves, init, want_fun, k)
    finally:
        eng.set_option(_capi.QT_OPT_SHOTS_CHECK, 1)
        eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, 1)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    first = runs[1, 1024, "lin", True]
    print("status of the all-zero trial:", {k: int(v["status"][i_zero]) for k, v in runs.items()})
    for waves in (1024, 0):
        for init in ("lin", "mixed"):
            ref = runs[1, waves, init, True]["status"][i_zero]
            for spec in (1, 0):
                for want_fun in (True, False):
                    assert runs[spec, waves, init, want_fun]["status"][i_zero] == ref, (spec, waves, init, want_fun)
    assert first["status"][i_zero] != 0
