"""GPU: the front and the first evaluation of the n = 3 specialised MLE kernels after the integer front of load_freq
(counts below 2^22 are summed as 32-bit integers, decided per wavefront), the dropped second store of the Bloch element
in nll_grad and the two ballots in place of the first gradient norm.  None of it touches a floating-point operation, so
every check is np.array_equal against the generic instantiation of the same kernels (QT_OPT_MLE_SPECIALISE = 0): rho,
nit, nfev, fun, status.

The launches are small, where a wrong lane, wave or scratch shows: partial workgroups, padding waves (lanes 24 - 63 of a
wavefront recompute row l + 128 in place of the missing row l + 192), twins beside dead lanes, a twin that takes its
trial into the BFGS loop, two scratch sizes (max_iter moves every base behind a trial's scratch), trials that iterate
past the pairs kept in LDS, and counts on both sides of 2^22 and beyond 2^32."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

ROUTES = ("hw", "fused", "split")


def _engine(shots):
    import quantpy_amd as qp

    eng = qp.get_engine(3)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * shots)
    return eng


def _run(eng, counts, route, init="lin", max_iter=100, specialise=True):
    """One device-pointer call -> dict of host arrays.  route: the twin kernel, k_mle_fused(_mixed), or the split pair."""
    import torch
    from quantpy_amd import _capi

    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    nit, nfev, status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda")
    rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
    try:
        eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, 1 if specialise else 0)
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1 if route == "hw" else 0)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 0 if route == "split" else 1024)
        eng.mle_dev(cd, rho, init=init, max_iter=max_iter, nit=nit, nfev=nfev, fun=fun, status=status)
        took_hw, took_spec = eng.mle_helper_wave, eng.mle_specialised
        eng.sync()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_SPECIALISE, 1)
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    assert took_hw == (route == "hw" and init == "lin"), (route, init, took_hw)
    assert took_spec == specialise, (route, init, specialise, took_spec)
    return dict(rho=rho.cpu().numpy().view(np.float64), nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(), fun=fun.cpu().numpy(),
                status=status.cpu().numpy())


def _equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def _ginibre(rng, rank):
    g = rng.standard_normal((8, rank)) + 1j * rng.standard_normal((8, rank))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _draw(oracle, rho, shots, seed, n):
    povm = oracle.measurement_matrix("proj-set", 3)
    bloch = oracle.bloch_from_matrix(rho)
    np.random.seed(seed)
    return np.stack([oracle.sample_counts(povm, bloch, np.ones(27) * shots) for _ in range(n)]).astype(np.int64)


@pytest.fixture(scope="module")
def classes():
    """Five trials at 1e5 shots and their generic results: the first four classes of tests/golden/chain_diet_bits.npz
    (positive definite; one negative pivot, the last: the twin lifts and takes the trial over; one negative pivot that
    is not the last: the twin declines and the trial falls back to its own sweep; two negative pivots: the
    eigensolver) and the lifted one again, alone in the second workgroup beside three padding waves."""
    counts = load_golden("chain_diet_bits")["counts"][[0, 1, 2, 3, 1]]
    return counts, _run(_engine(100000), counts, "fused", specialise=False)


@pytest.fixture(scope="module")
def low_shot():
    """The five rank-1 trials at 1000 shots of tests/golden/mle_diet_bits.npz: 11 - 13 iterations from 'lin', and from
    the mixed start more than the 24 (k_mle_fused) / 16 (twin kernel) pairs that stay in LDS."""
    return load_golden("mle_diet_bits")["n3_rank1_lowshot/counts"]


@pytest.mark.parametrize("route", ROUTES)
def test_partial_workgroup_every_class(classes, route):
    counts, ref = classes
    assert ref["status"].tolist() == [0] * 5
    _equal(_run(_engine(100000), counts, route), ref, route)


@pytest.mark.parametrize("route", ROUTES)
def test_iterating_from_lin(low_shot, route):
    """Trials that leave the start with a gradient above gtol: the ballots send them into the BFGS loop."""
    eng = _engine(1000)
    ref = _run(eng, low_shot, "fused", specialise=False)
    assert (ref["nit"] > 0).all() and (ref["status"] == 0).all(), (ref["nit"], ref["status"])
    _equal(_run(eng, low_shot, route), ref, route)


def test_twin_that_owns_its_trial_iterates(oracle):
    """A rank-7 state at 1000 shots: the linear inversion has ONE negative eigenvalue, met at the last pivot -- the class
    the twin lifts -- and the lifted start is not the optimum, so the wave that goes into the BFGS loop is the twin, in
    its own scratch.  (A rank-1 state's linear inversion has three or four negative
    eigenvalues at every shot count: its trials iterate, test_iterating_from_lin, but on the first wave.)"""
    povm = oracle.measurement_matrix("proj-set", 3)
    counts = _draw(oracle, _ginibre(np.random.default_rng(11), 7), 1000, 9, 3)
    for c in counts:
        lam = np.linalg.eigvalsh(np.asarray(oracle.lin_estimate(c, povm, physical=False)))
        assert (lam < 0).sum() == 1, lam
    eng = _engine(1000)
    ref = _run(eng, counts, "fused", specialise=False)
    assert (ref["nit"] > 0).all() and (ref["status"] == 0).all(), (ref["nit"], ref["status"])
    for route in ROUTES:
        _equal(_run(eng, counts, route), ref, route)


@pytest.mark.parametrize("max_iter", [100, 256])
def test_mixed_start_two_scratch_sizes(low_shot, max_iter):
    """max_iter sizes the line-search and pair slots behind a trial's scratch: every scratch base differs between the two
    launches; the results do not."""
    eng = _engine(1000)
    counts = low_shot[:3]
    ref = _run(eng, counts, "fused", init="mixed", max_iter=max_iter, specialise=False)
    assert (ref["nit"] > 16).any() and (ref["nit"] < max_iter).all() and (ref["status"] == 0).all(), (ref["nit"], ref["status"])
    for route in ("fused", "split"):
        _equal(_run(eng, counts, route, init="mixed", max_iter=max_iter), ref, (route, max_iter))
    if max_iter == 256:  # the trials stop on their own: the iteration cap is not part of a result
        _equal(ref, _run(eng, counts, "fused", init="mixed", max_iter=100, specialise=False), "max_iter")


def test_same_launch_twice(classes, low_shot):
    counts, _ = classes
    for shots, c, init in ((100000, counts, "lin"), (1000, low_shot, "lin"), (1000, low_shot[:3], "mixed")):
        eng = _engine(shots)
        for route in ("hw", "fused") if init == "lin" else ("fused",):
            _equal(_run(eng, c, route, init=init), _run(eng, c, route, init=init), (route, init))


def _rescaled(base, n, pin):
    """`base` (27, 8) rescaled to n shots per setting, every count below 2^22 where n allows it, then outcome 0 of setting
    0 set to `pin` at the cost of that setting's other outcomes."""
    out = np.empty_like(base)
    for s in range(27):
        want = pin if s == 0 else None
        rest = n - (want or 0)
        w = base[s].astype(np.float64).copy()
        if want is not None:
            w[0] = 0.0
        c = np.floor(w / w.sum() * rest).astype(np.int64)
        cap = (1 << 22) - 1
        if rest <= 7 * cap:  # (level the rows that would pass 2^22 - 1: the trial is about ONE count at the edge)
            for _ in range(8):
                over = np.maximum(c - cap, 0)
                c -= over
                free = (c < cap) & (w > 0)
                c[np.flatnonzero(free)[np.argmin(c[free])]] += over.sum()
        c[np.argmax(w)] += rest - c.sum()
        if want is not None:
            c[0] = want
        out[s] = c
    assert (out.sum(axis=1) == n).all() and (out >= 0).all()
    return out


def test_integer_front_and_its_edges(classes):
    """load_freq sums counts below 2^22 as 32-bit integers, decided per wavefront.  Three trials in one workgroup: every
    count below 2^22 and one of them 2^22 - 1 (the integer sums); the same with that count at 2^22 (the sums on
    doubles); a count above 2^32.  The registered shots per setting are the first two trials'; the third has 2^11 times
    as many in every setting, which the shots check accepts (it compares proportions)."""
    base = classes[0][0]
    n = 1 << 23
    edge, past = _rescaled(base, n, (1 << 22) - 1), _rescaled(base, n, 1 << 22)
    huge = _rescaled(base, n << 11, (1 << 32) + 5)
    assert edge.max() == (1 << 22) - 1 and past.max() == 1 << 22 and (past >= 1 << 22).sum() == 1
    assert huge.max() > 1 << 32
    counts = np.stack([edge, past, huge])
    eng = _engine(n)
    ref = _run(eng, counts, "fused", specialise=False)
    assert (ref["status"] == 0).all(), ref["status"]
    for route in ROUTES:
        _equal(_run(eng, counts, route), ref, route)
