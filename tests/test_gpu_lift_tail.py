"""GPU: the end of the lift and the early outputs of the one-launch n = 3 MLE.  The certificate of
lift_single_negative leaves through one test with its result formed beside the residual check (so `out` is written
on a refusal too), and mle_fused_body stores the start matrix and the scalars of the common case (nit 0, nfev 1,
status 0) in front of the first evaluation and writes behind it only what differs.  (Three more re-orderings of the same
chain ran through these tests and were dropped on their timing: DESIGN 4.1.)  No floating-point operation moves, so every check is np.array_equal of all a
launch writes, the kernel with twin wavefronts (QT_OPT_MLE_HELPER_WAVE = 1) against the one without (0), and both
against the split pair k_mle_start / k_mle_bfgs where the early outputs are the subject: that pair stores once, at the end.

Every output buffer is filled with sentinels first (rho: NaN, nit / nfev / status: 7 / 8 / 9), so a store that is
skipped shows as much as one that is wrong.  The trial classes are the recipes of tests/test_gpu_mle_helper_lift.py and
tests/test_gpu_lane_constants.py; every test asserts from the CPU oracle's linear inversion that its trials are of the
class it names.  n = 3, 'proj-set', at most 16 trials a launch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 8
SENT = dict(nit=7, nfev=8, status=9)


def _ginibre(rng, d, rank=None):
    g = rng.standard_normal((d, rank or d)) + 1j * rng.standard_normal((d, rank or d))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _sweep(a):
    """L S L^dagger elimination carried on past non-positive pivots: (number of them, index of the first or d - 1)."""
    a = np.array(a, dtype=np.complex128)
    neg, kneg = 0, D - 1
    for k in range(D):
        akk = a[k, k].real
        if not akk > 0.0:
            if neg == 0:
                kneg = k
            neg += 1
        col = a[k + 1:, k].copy()
        a[k + 1:, k + 1:] -= np.outer(col, col.conj()) / akk
    return neg, kneg


def _classes(oracle, povm, counts):
    """Per trial: (negative eigenvalues, neg, kneg, |lam_1| / lam_2) of the unprojected linear-inversion estimate."""
    rows = []
    for c in counts:
        lin = np.asarray(oracle.lin_estimate(c, povm, physical=False))
        lam = np.linalg.eigvalsh(lin)
        neg, kneg = _sweep(lin)
        rows.append((int((lam < 0).sum()), neg, kneg, abs(lam[0]) / lam[1] if lam[1] > 0 else np.inf))
    return rows


def _draw(oracle, povm, rho, shots, seed, n):
    bloch = oracle.bloch_from_matrix(rho)
    np.random.seed(seed)
    return np.stack([oracle.sample_counts(povm, bloch, np.ones(27) * shots) for _ in range(n)]).astype(np.int64)


@pytest.fixture(scope="module")
def data(oracle):
    """Five sets -> counts, shots per setting, classes."""
    povm = oracle.measurement_matrix("proj-set", 3)
    sets = {}
    # the benchmark's stream, trials 10 .. 18: positive definite and "go"
    sets["bench"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(1234), D), 100000, 7, 19)[10:], 100000)
    # no weight on |0>: the FIRST pivot is the non-positive one
    g = _ginibre(np.random.default_rng(5), D)
    p = np.eye(D)
    p[0, 0] = 0.0
    pgp = p @ g @ p
    sets["pivot0"] = (_draw(oracle, povm, pgp / np.trace(pgp), 100000, 21, 12), 100000)
    # rank 6 at 1e4 shots: |lam_1| of the size of lam_2: the lift runs to its end, or to its third squaring, and declines
    sets["rank6"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(106), D, rank=6), 10000, 32, 20), 10000)
    # rank 1 at 1e3 shots: several negative eigenvalues
    sets["rank1"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(77), D, rank=1), 1000, 8, 4), 1000)
    # rank 7 at 1e3 shots: one negative eigenvalue at the last pivot, and the lifted start is not the optimum
    sets["rank7"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(11), D, rank=7), 1000, 9, 3), 1000)
    return {k: {"counts": c, "shots": s, "cls": _classes(oracle, povm, c)} for k, (c, s) in sets.items()}


def _pick(s, want, n=None):
    """The trials of set `s` whose class satisfies `want(eigs, neg, kneg, ratio)`."""
    idx = [t for t, c in enumerate(s["cls"]) if want(*c)]
    return s["counts"][idx[:n]], idx[:n]


@pytest.fixture(scope="module")
def eng():
    import quantpy_amd as qp

    return qp.get_engine(3)


def _set_povm(eng, shots):
    import quantpy_amd as qp

    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * shots)


class _Buffers:
    """Device buffers of `rows` >= B rows, filled with the sentinels."""

    def __init__(self, counts, rows=None, with_fun=False, dist_centre=None, null=()):
        import torch

        self.b = counts.shape[0]
        rows = rows or self.b
        self.cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
        self.out = {k: None if k in null else torch.full((rows,), v, dtype=torch.int32, device="cuda") for k, v in SENT.items()}
        self.fun = torch.full((rows,), np.nan, dtype=torch.float64, device="cuda") if with_fun else None
        self.cen = self.dist = self.rho = None
        if dist_centre is None:
            self.rho = torch.full((rows, D, D), complex(np.nan, np.nan), dtype=torch.complex128, device="cuda")
        else:
            self.cen = torch.from_numpy(np.ascontiguousarray(dist_centre, dtype=np.complex128)).cuda()
            self.dist = torch.full((rows,), np.nan, dtype=torch.float64, device="cuda")

    def host(self):
        """Everything a launch may write, as raw 64- or 32-bit words (a NaN sentinel compares equal to itself)."""
        got = {k: v.cpu().numpy() for k, v in self.out.items() if v is not None}
        for k in ("rho", "dist", "fun"):
            t = getattr(self, k)
            if t is not None:
                got[k] = t.cpu().numpy().view(np.uint64)
        return got


def _launch(eng, buf, route, max_iter=100):
    """One device-pointer launch into `buf`: the twin kernel ('hw'), k_mle_fused ('fused') or the split pair ('split')."""
    from quantpy_amd import _capi

    kw = dict(max_iter=max_iter, nit=buf.out["nit"], nfev=buf.out["nfev"], fun=buf.fun, status=buf.out["status"])
    try:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1 if route == "hw" else 0)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 0 if route == "split" else 1024)
        if buf.cen is None:
            eng.mle_dev(buf.cd, buf.rho, **kw)
        else:
            eng.mle_dist_dev(buf.cd, buf.cen, buf.dist, rho=None, **kw)
        took = eng.mle_helper_wave
        eng.sync()
    finally:
        eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        eng.set_option(_capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    assert took == (route == "hw"), (route, took)
    return buf.host()


def _equal(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def _on_off(eng, counts, routes=("hw", "fused"), max_iter=100, **kw):
    """The same trials through each route into fresh sentinel-filled buffers: all equal; returns the first."""
    got = [_launch(eng, _Buffers(counts, **kw), r, max_iter) for r in routes]
    for g, r in zip(got[1:], routes[1:]):
        _equal(got[0], g, r)
    b = counts.shape[0]
    for k, v in SENT.items():
        if k in got[0]:
            assert (got[0][k][:b] != v).all(), (k, got[0][k])  # every live row was written
    if "rho" in got[0]:
        assert not np.isnan(got[0]["rho"][:b].view(np.float64)).any()
    return got[0]


# ---- the trial classes through the lift's one exit ----------------------------------------------------------------

def test_positive_definite(eng, data):
    counts, idx = _pick(data["bench"], lambda e, n, k, r: e == 0 and n == 0)
    assert len(idx) >= 7, data["bench"]["cls"]
    _set_povm(eng, 100000)
    on = _on_off(eng, counts)
    assert (on["status"] == 0).all() and (on["nit"] == 0).all() and (on["nfev"] == 1).all(), on


def test_go(eng, data):
    """One negative pivot, the last, and a fast ratio: the twin lifts, claims and owns the trial."""
    counts, idx = _pick(data["bench"], lambda e, n, k, r: (e, n, k) == (1, 1, 7) and r < 0.5)
    assert len(idx) >= 2, data["bench"]["cls"]
    _set_povm(eng, 100000)
    for b in (len(idx), 1):
        on = _on_off(eng, counts[:b])
        assert (on["status"] == 0).all(), on["status"]


def test_refused_behind_the_squarings_then_iterates(eng, data):
    """|lam_1| > lam_2: the squarings certify the WRONG direction, lam comes out positive (or the residual large): the one
    exit refuses with `out` already written, and nobody reads it."""
    s = data["rank6"]
    for t in (0, 1, 17):
        assert s["cls"][t][:3] == (1, 1, 7) and s["cls"][t][3] > 1.2, (t, s["cls"][t])
    _set_povm(eng, s["shots"])
    on = _on_off(eng, s["counts"][[0, 1, 17]], routes=("hw", "fused", "split"))
    assert (on["nit"] > 0).sum() >= 2 and (on["status"] == 0).all(), (on["nit"], on["status"])


def test_refused_at_the_third_squaring_then_iterates(eng, data):
    s = data["rank6"]
    assert s["cls"][18][:3] == (1, 1, 7) and 0.85 < s["cls"][18][3] < 1.0, s["cls"][18]
    _set_povm(eng, s["shots"])
    on = _on_off(eng, s["counts"][[18]], routes=("hw", "fused", "split"))
    assert on["nit"][0] > 0 and on["status"][0] == 0, (on["nit"], on["status"])


def test_several_negative_eigenvalues(eng, data):
    s = data["rank1"]
    assert all(3 <= e <= 4 for e, _, _, _ in s["cls"]), s["cls"]
    _set_povm(eng, s["shots"])
    _on_off(eng, s["counts"], routes=("hw", "fused", "split"))


def test_wrong_pivot_order(eng, data):
    counts, idx = _pick(data["pivot0"], lambda e, n, k, r: (e, n, k) == (1, 1, 0))
    assert len(idx) >= 5, data["pivot0"]["cls"]
    _set_povm(eng, 100000)
    _on_off(eng, counts)


# ---- early outputs ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def five(data):
    """Five trials at 1e5 shots, one per class: positive definite, go, refused (rank 6), several negative eigenvalues
    (rank 1), first pivot.  (Counts scaled to the launch's shot count: the frequencies, hence the classes, stay.)"""
    b = data["bench"]
    pd, _ = _pick(b, lambda e, n, k, r: e == 0 and n == 0, 1)
    go, _ = _pick(b, lambda e, n, k, r: (e, n, k) == (1, 1, 7) and r < 0.5, 1)
    p0, _ = _pick(data["pivot0"], lambda e, n, k, r: (e, n, k) == (1, 1, 0), 1)
    assert len(pd) == len(go) == len(p0) == 1
    return np.concatenate([pd, go, data["rank6"]["counts"][[0]] * 10, data["rank1"]["counts"][[0]] * 100, p0])


ROUTES3 = ("hw", "fused", "split")


def test_rows_behind_the_batch_keep_their_sentinels(eng, five):
    _set_povm(eng, 100000)
    got = _on_off(eng, five, routes=ROUTES3, rows=8)
    assert got["nit"].shape == (8,)
    for k, v in SENT.items():
        assert (got[k][5:] == v).all(), (k, got[k])
    nan_bits = np.array([np.nan]).view(np.uint64)[0]
    assert (got["rho"][5:] == nan_bits).all()
    assert (got["status"][:5] == 0).all(), got["status"]


def test_lin_start_that_iterates(eng, data):
    """The twin owns these trials and takes them into the BFGS loop: what it stored early is overwritten by the loop."""
    s = data["rank7"]
    assert all(c[0] == 1 for c in s["cls"]), s["cls"]
    _set_povm(eng, s["shots"])
    on = _on_off(eng, s["counts"], routes=ROUTES3)
    assert (on["nit"] > 0).all() and (on["status"] == 0).all(), (on["nit"], on["status"])


def test_wrong_shot_total(eng, five):
    counts = five.copy()
    counts[1, 0, 0] += 1  # the "go" trial
    counts[3, 5, 2] += 1
    _set_povm(eng, 100000)
    on = _on_off(eng, counts, routes=ROUTES3)
    assert on["status"].tolist() == [0, 5, 0, 5, 0], on["status"]


def test_no_iterations(eng, five):
    _set_povm(eng, 100000)
    on = _on_off(eng, five, routes=ROUTES3, max_iter=0)
    assert (on["nit"] == 0).all() and (on["status"] != 0).all(), (on["nit"], on["status"])  # (3: the iteration cap)


def test_fun_requested(eng, five):
    _set_povm(eng, 100000)
    on = _on_off(eng, five, routes=ROUTES3, with_fun=True)
    assert not np.isnan(on["fun"].view(np.float64)).any()


def test_distance_entry(eng, five):
    _set_povm(eng, 100000)
    on = _on_off(eng, five, routes=ROUTES3, dist_centre=_ginibre(np.random.default_rng(5), D))
    assert not np.isnan(on["dist"].view(np.float64)).any()


@pytest.mark.parametrize("null", ["nit", "nfev", "status"])
def test_one_scalar_output_null(eng, five, null):
    _set_povm(eng, 100000)
    full = _launch(eng, _Buffers(five), "fused")
    on = _on_off(eng, five, routes=ROUTES3, null=(null,))
    assert null not in on
    for k in on:
        assert np.array_equal(on[k], full[k]), k


def test_same_launch_twice(eng, five, data):
    """The second launch finds the first one's results in the buffers, and its early stores write over them."""
    for shots, counts in ((100000, five), (data["rank7"]["shots"], data["rank7"]["counts"])):
        _set_povm(eng, shots)
        ref = _launch(eng, _Buffers(counts, rows=8), "fused")
        for route in ("hw", "fused"):
            buf = _Buffers(counts, rows=8)
            first = _launch(eng, buf, route)
            second = _launch(eng, buf, route)
            _equal(first, second, route)
            _equal(second, ref, route)
