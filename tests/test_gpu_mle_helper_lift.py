"""GPU: the speculative lift on the helper wavefront of the one-launch n = 3 MLE (k_mle_fused_hw,
QT_OPT_MLE_HELPER_WAVE = 1) against the launch without helpers (k_mle_fused, option 0) on one engine.  The helper lifts
every trial's linear-inversion matrix before the first Cholesky sweep has said whether that is wanted; the sweep's
verdict lets it go on (one negative pivot, the last), or sends it home (everything else).  No floating-point operation
or its order changes, so "equal" below is np.array_equal on everything a launch writes.  Every call is a device-pointer
call, and every launch sets the option itself and puts 1 back.

The class of a trial is computed here on the CPU from its unprojected linear-inversion estimate: the number of
negative eigenvalues and, from an L S L^dagger sweep, the number of non-positive pivots `neg` and the first of them
`kneg` -- what the kernel's first sweep sees.  The minimum counts asserted in test_classes are those the four recipes
gave on the CPU oracle, so that a drift of the inputs cannot hollow the tests out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 8


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
    """The four sets: counts, shots per setting, classes."""
    povm = oracle.measurement_matrix("proj-set", 3)
    sets = {}
    # 1: the benchmark's stream, trials 10 .. 18
    sets["bench"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(1234), D), 100000, 7, 19)[10:], 100000)
    # 2: a state with no weight on |0>: the FIRST pivot is the one that goes non-positive
    g = _ginibre(np.random.default_rng(5), D)
    p = np.eye(D)
    p[0, 0] = 0.0
    pgp = p @ g @ p
    sets["pivot0"] = (_draw(oracle, povm, pgp / np.trace(pgp), 100000, 21, 12), 100000)
    # 3: rank 6 at 1e4 shots: |lam_1| is of the size of lam_2, the lift runs to its end and declines
    sets["rank6"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(106), D, rank=6), 10000, 32, 20), 10000)
    # 4: rank 1 at 1e3 shots: several negative eigenvalues
    sets["rank1"] = (_draw(oracle, povm, _ginibre(np.random.default_rng(77), D, rank=1), 1000, 8, 4), 1000)
    return {k: {"counts": c, "shots": s, "cls": _classes(oracle, povm, c)} for k, (c, s) in sets.items()}


@pytest.fixture(scope="module")
def eng():
    import quantpy_amd as qp

    return qp.get_engine(3)


def _set_povm(eng, shots):
    import quantpy_amd as qp

    eng.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * shots)


class _Launch:
    """The device buffers of a launch, so that a second launch can write into the same ones."""

    def __init__(self, eng, counts, with_fun=False, dist_centre=None):
        import torch

        b = counts.shape[0]
        self.eng, self.with_fun = eng, with_fun
        self.cd = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
        self.nit, self.nfev, self.status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        self.fun = torch.zeros(b, dtype=torch.float64, device="cuda") if with_fun else None
        self.cen = None
        if dist_centre is None:
            self.rho = torch.zeros((b, D, D), dtype=torch.complex128, device="cuda")
        else:
            self.cen = torch.from_numpy(np.ascontiguousarray(dist_centre, dtype=np.complex128)).cuda()
            self.dist = torch.zeros(b, dtype=torch.float64, device="cuda")

    def run(self, helper, max_iter=100):
        """One launch with the option at `helper`: everything it writes, and whether it was the kernel with helpers."""
        from quantpy_amd import _capi

        eng, out = self.eng, {}
        kw = dict(max_iter=max_iter, nit=self.nit, nfev=self.nfev, fun=self.fun, status=self.status)
        try:
            eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, helper)
            if self.cen is None:
                eng.mle_dev(self.cd, self.rho, **kw)
            else:
                eng.mle_dist_dev(self.cd, self.cen, self.dist, rho=None, **kw)
            took = eng.mle_helper_wave
            eng.sync()
        finally:
            eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        if self.cen is None:
            out["rho"] = self.rho.cpu().numpy().view(np.float64)
        else:
            out["dist"] = self.dist.cpu().numpy()
        out.update(nit=self.nit.cpu().numpy(), nfev=self.nfev.cpu().numpy(), status=self.status.cpu().numpy())
        if self.with_fun:
            out["fun"] = self.fun.cpu().numpy()
        return out, took


def _equal(on, off):
    assert on.keys() == off.keys()
    for k in on:
        assert np.array_equal(on[k], off[k]), (k, on[k], off[k])
    assert (on["status"] != -7).all() and (on["nit"] != -7).all() and (on["nfev"] != -7).all()


def _same_bits(eng, counts, max_iter=100, **kw):
    on, took_on = _Launch(eng, counts, **kw).run(1, max_iter)
    off, took_off = _Launch(eng, counts, **kw).run(0, max_iter)
    assert took_on and not took_off
    _equal(on, off)
    return on


def test_classes(data):
    """The sets hold what the tests below are about (counts: what the CPU oracle gave for these recipes)."""
    c = data["bench"]["cls"]
    assert sum(1 for e, n, k, _ in c if e == 0 and n == 0) >= 7, c            # positive definite: abort, never waits
    assert sum(1 for e, n, k, _ in c if e == 1 and n == 1 and k == 7) >= 2, c  # go
    c = data["pivot0"]["cls"]
    assert sum(1 for e, n, k, _ in c if e == 1 and n == 1 and k == 0) >= 5, c  # wrong pivot order: abort, own lift
    assert sum(1 for e, n, k, _ in c if e == 1 and n == 1 and k == 7) >= 1, c
    assert sum(1 for e, n, k, _ in c if e == 0) >= 6, c
    c = data["rank6"]["cls"]
    for t in (0, 1, 17):  # go, and the lift finds the wrong direction dominant: refused after the squarings
        assert c[t][:3] == (1, 1, 7) and c[t][3] > 1.2, (t, c[t])
    assert c[18][:3] == (1, 1, 7) and 0.85 < c[18][3] < 1.0, c[18]  # go, refused at the third squaring
    for t in (3, 5, 15, 16, 19):
        assert c[t][1] == 1 and c[t][2] in (5, 6), (t, c[t])
    c = data["rank1"]["cls"]
    assert all(3 <= e <= 4 for e, _, _, _ in c), c  # the eigensolver


@pytest.mark.parametrize("b", [9, 1, 5])
def test_benchmark_classes(eng, data, b):
    s = data["bench"]
    _set_povm(eng, s["shots"])
    on = _same_bits(eng, s["counts"][:b])
    assert (on["status"] == 0).all(), on["status"]


def test_wrong_pivot_order_aborts(eng, data):
    s = data["pivot0"]
    _set_povm(eng, s["shots"])
    _same_bits(eng, s["counts"])


def test_refused_lift_then_bfgs(eng, data):
    """The lift runs to its end on the helper and declines; the trials iterate afterwards, over the hand-off region."""
    s = data["rank6"]
    _set_povm(eng, s["shots"])
    on = _same_bits(eng, s["counts"], with_fun=True)
    print("nit", on["nit"], "nfev", on["nfev"])
    # most of the named trials of each class iterate (on the recipe's data: 3 of 4 and 4 of 5), not one that carries the check
    assert (on["nit"][[0, 1, 17, 18]] > 0).sum() >= 3 and (on["nit"][[3, 5, 15, 16, 19]] > 0).sum() >= 3, on["nit"]


def test_several_negative_eigenvalues(eng, data):
    s = data["rank1"]
    _set_povm(eng, s["shots"])
    _same_bits(eng, s["counts"])


def _mixed(data):
    """All four sets, interleaved so that a workgroup (4 consecutive trials) holds different classes; the counts scaled to
    1e5 shots per setting, the one shot count a launch has."""
    scaled = [data[k]["counts"] * (100000 // data[k]["shots"]) for k in ("bench", "pivot0", "rank6", "rank1")]
    n = max(len(s) for s in scaled)
    rows = [s[t] for t in range(n) for s in scaled if t < len(s)]
    return np.stack(rows)


def test_all_classes_in_one_launch(eng, data):
    counts = _mixed(data)
    assert counts.shape[0] == 45
    _set_povm(eng, 100000)
    on = _same_bits(eng, counts)
    print("nit", on["nit"], "status", on["status"])


def test_same_outputs_twice(eng, data):
    """The words of the hand-off are set up by every launch: a second launch into the same buffers gives the same."""
    counts = _mixed(data)
    _set_povm(eng, 100000)
    launch = _Launch(eng, counts, with_fun=True)
    first, took = launch.run(1)
    second, took2 = launch.run(1)
    assert took and took2
    _equal(first, second)
    off, _ = _Launch(eng, counts, with_fun=True).run(0)
    _equal(second, off)


def test_no_iterations(eng, data):
    counts = _mixed(data)
    _set_povm(eng, 100000)
    on = _same_bits(eng, counts, max_iter=0)
    assert (on["nit"] == 0).all()


def test_with_fun(eng, data):
    s = data["bench"]
    _set_povm(eng, s["shots"])
    _same_bits(eng, s["counts"], with_fun=True)


def test_distance_entry(eng, data):
    counts = _mixed(data)[:20]
    _set_povm(eng, 100000)
    _same_bits(eng, counts, dist_centre=_ginibre(np.random.default_rng(5), D))
