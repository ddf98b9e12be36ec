"""GPU: the twin wavefront of the one-launch n = 3 MLE (k_mle_fused_hw, QT_OPT_MLE_HELPER_WAVE = 1) against the launch
without twins (k_mle_fused, option 0) on one engine.  The twin reads its trial's counts itself and runs load_freq and
lin_invert on a scratch of its own behind the trials' scratches, so the launch keeps 16 instead of 24 (s, y) pairs per
trial in LDS.  No floating-point operation or its order changes, and where a pair lives changes no bit, so "equal" below
is np.array_equal on everything a launch writes: rho, nit, nfev, status and fun.  Every call is a device-pointer call, and
every launch sets the option itself and puts 1 back.

The inputs are trials 10 .. 18 of the benchmark's stream (the "bench" recipe of test_gpu_mle_helper_lift.py).  On the
CPU oracle (solver="port") with tol = 1e-6 and max_iter = 100, trials 2 and 8 of that slice are the class the twin's
lift serves (one negative eigenvalue, one non-positive pivot, the last; |lam_1| / lam_2 = 0.01 and 0.06) and iterate 69
and 74 times; the positive-definite ones iterate 50 to 100 times.  So both classes cross 16 and 24 pairs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 8
GO = (2, 8)  # the go-class trials of the slice (asserted on the CPU in test_go_class)
SENTINEL = -7


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


@pytest.fixture(scope="module")
def data(oracle):
    """Counts of the nine trials and, per trial, (negative eigenvalues, neg, kneg) of the unprojected linear inversion."""
    povm = oracle.measurement_matrix("proj-set", 3)
    g = np.random.default_rng(1234)
    m = g.standard_normal((D, D)) + 1j * g.standard_normal((D, D))
    rho = m @ m.conj().T
    rho /= np.trace(rho)
    bloch = oracle.bloch_from_matrix(rho)
    np.random.seed(7)
    counts = np.stack([oracle.sample_counts(povm, bloch, np.ones(27) * 100000) for _ in range(19)]).astype(np.int64)[10:]
    cls = []
    for c in counts:
        lin = np.asarray(oracle.lin_estimate(c, povm, physical=False))
        cls.append((int((np.linalg.eigvalsh(lin) < 0).sum()),) + _sweep(lin))
    return {"counts": counts, "cls": cls}


@pytest.fixture(scope="module")
def eng():
    import quantpy_amd as qp

    e = qp.get_engine(3)
    e.set_povm(qp.generate_measurement_matrix("proj-set", 3), np.ones(27) * 100000)
    return e


class _Launch:
    """Device buffers with four rows of sentinel behind the B rows a launch may write; the launch gets views of the B."""

    def __init__(self, counts):
        import torch

        b = self.b = counts.shape[0]
        self.cd = torch.from_numpy(np.ascontiguousarray(counts)).cuda()
        self.rho = torch.full((b + 4, D, D), complex(SENTINEL, SENTINEL), dtype=torch.complex128, device="cuda")
        self.nit, self.nfev, self.status = (torch.full((b + 4,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3))
        self.fun = torch.full((b + 4,), float(SENTINEL), dtype=torch.float64, device="cuda")

    def run(self, eng, helper, max_iter, tol):
        """One launch with the option at `helper`: what it wrote, the rows behind, and whether the twins' kernel ran."""
        from quantpy_amd import _capi

        b = self.b
        try:
            eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, helper)
            eng.mle_dev(self.cd, self.rho[:b], max_iter=max_iter, tol=tol, nit=self.nit[:b], nfev=self.nfev[:b],
                        fun=self.fun[:b], status=self.status[:b])
            took = eng.mle_helper_wave
            eng.sync()
        finally:
            eng.set_option(_capi.QT_OPT_MLE_HELPER_WAVE, 1)
        full = dict(rho=self.rho.cpu().numpy().view(np.float64), nit=self.nit.cpu().numpy(), nfev=self.nfev.cpu().numpy(),
                    status=self.status.cpu().numpy(), fun=self.fun.cpu().numpy())
        for k, v in full.items():  # no word behind row B is touched
            assert (v[b:] == SENTINEL).all(), (k, v[b:])
        return {k: v[:b] for k, v in full.items()}, took


def _equal(on, off):
    assert on.keys() == off.keys()
    for k in on:
        assert np.array_equal(on[k], off[k]), (k, on[k], off[k])
    assert (on["status"] != SENTINEL).all() and (on["nit"] != SENTINEL).all() and (on["nfev"] != SENTINEL).all()


def _same_bits(eng, counts, max_iter=100, tol=1e-6):
    on, took_on = _Launch(counts).run(eng, 1, max_iter, tol)
    off, took_off = _Launch(counts).run(eng, 0, max_iter, tol)
    assert took_on and not took_off
    _equal(on, off)
    return on


def test_go_class(data):
    """Trials 2 and 8 are the class the twin lifts; the other seven are positive definite."""
    c = data["cls"]
    for t in GO:
        assert c[t] == (1, 1, D - 1), (t, c)
    assert sum(1 for e, n, _ in c if e == 0 and n == 0) == 7, c


def test_iterates_past_the_lds_pairs(eng, data):
    """Lifted and positive-definite trials iterate past pair 16 (this kernel's LDS pairs) and pair 24 (k_mle_fused's)."""
    on = _same_bits(eng, data["counts"])
    print("nit", on["nit"], "nfev", on["nfev"], "status", on["status"])
    assert (on["nit"][list(GO)] > 24).all(), on["nit"]
    pd = [t for t, (e, n, _) in enumerate(data["cls"]) if e == 0 and n == 0]
    assert (on["nit"][pd] > 24).all(), on["nit"]


def test_largest_max_iter_of_the_one_launch_path(eng, data):
    """max_iter = 256: the layout with the twins' scratches fits the LDS of a CU, and the twins' kernel is what runs."""
    on = _same_bits(eng, data["counts"], max_iter=256, tol=1e-9)  # (_same_bits asserts eng.mle_helper_wave)
    print("nit", on["nit"], "status", on["status"])


@pytest.mark.parametrize("b", [1, 3, 4, 5])
def test_go_trial_last(eng, data, b):
    """The last trial of the batch is a go-class one; at b = 1, 3, 5 it sits in a partial workgroup beside dead trials,
    whose twins run too.  (_Launch.run checks the rows behind the batch.)"""
    last = GO[0] if b <= 3 else GO[1]
    on = _same_bits(eng, data["counts"][last + 1 - b:last + 1])
    assert on["nit"].shape == (b,) and on["nit"][-1] > 24, on["nit"]


def test_same_launch_twice(eng, data):
    """Every launch sets the link words up itself: a second launch into the same buffers gives the same."""
    launch = _Launch(data["counts"])
    first, took = launch.run(eng, 1, 100, 1e-6)
    second, took2 = launch.run(eng, 1, 100, 1e-6)
    assert took and took2
    _equal(first, second)
    off, _ = _Launch(data["counts"]).run(eng, 0, 100, 1e-6)
    _equal(second, off)
