"""The coverage study of the confidence polytope on the GPU (qt_polytope_confidence / qt_polytope_coverage,
quantpy_amd.tomography.polytopes) against tests/golden/polytope_coverage.npz: the reference's count_confidence and an
extended-precision evaluation of it, seeded runs of the reference's test_qst / test_qpt, and the tables the reference
published (Verification.ipynb, 10 000 trials per row).

The module `verification` is imported, never the names test_qst / test_qpt: pytest would collect them."""
import ctypes

import numpy as np
import pytest
from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = 1e-15
# Two bisections whose comparisons differ only where the confidence is within rounding of the level return midpoints of
# brackets (width (1 - 1e-10) / 2^33 = 1.16e-10) that both hold a root: <= 1.2e-10 apart plus the distance of the roots.
DELTA_TOL = 2.5e-10


@pytest.fixture(scope="module")
def gold():
    return load_golden("polytope_coverage")


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


@pytest.fixture(scope="module")
def eng(qp):
    return qp.get_engine(1)


@pytest.fixture(scope="module")
def polytopes():
    from quantpy_amd.tomography.polytopes import utils, verification

    return utils, verification


def study_object(qp, gold, name):
    key = f"study/{name}/"
    n = int(gold[key + "n_qubits"])
    if key + "rho" in gold.files:
        return "state", qp.Qobj(gold[key + "rho"]), {}
    channel = qp.channel.depolarizing(p=float(gold[key + "depolarizing_p"]), n_qubits=n)
    return "channel", channel, {"input_states": str(gold[key + "input_states"])}


def test_confidence_formula_cases(gold, eng):
    """|kernel - extended| <= 4 e_ref + 4e-16 per group, e_ref = the float64 reference's own distance from the
    extended-precision value over the group; exact zeros and ones are exact."""
    for name in gold["formula_groups"]:
        key = f"formula/{name}/"
        counts, shots, deltas = gold[key + "counts"], gold[key + "shots"], gold[key + "deltas"]
        ext = gold[key + "ext_hi"].astype(np.longdouble) + gold[key + "ext_lo"].astype(np.longdouble)
        ref, e_ref = gold[key + "ref"], float(gold[key + "e_ref"])
        got = eng.polytope_confidence(counts, shots, deltas)
        assert got.shape == ref.shape
        err = float(np.max(np.abs(got.astype(np.longdouble) - ext)))
        print(f"{name} {counts.shape[1:]}: e_ref {e_ref:.2e} kernel error {err:.2e} (bound {4 * e_ref + 4e-16:.2e})")
        assert err <= 4 * e_ref + 4e-16, (name, err, e_ref)
        assert np.array_equal(got[ref == 0.0], ref[ref == 0.0]), name
        assert np.array_equal(got[ref == 1.0], ref[ref == 1.0]), name
        # one widening row shared by all trials gives the same bits as the same row repeated per trial
        assert np.array_equal(eng.polytope_confidence(counts, shots, deltas[0])[0], got[0])


def test_coverage_seeded_studies(gold, qp, eng, polytopes):
    utils, verification = polytopes
    levels = gold["levels"]
    for name in gold["studies"]:
        key = f"study/{name}/"
        kind, obj, kw = study_object(qp, gold, name)
        shots = int(gold[key + "shots"])
        if kind == "state":
            probas, n_meas, truth = verification.qst_setup(obj, shots)
        else:
            probas, n_meas, truth = verification.qpt_setup(obj, shots, **kw)
        counts = gold[key + "counts"]
        trials = counts.shape[0]
        covered, deltas, hits = eng.polytope_coverage(counts, n_meas, levels, truth=truth, clip_b=kind == "state",
                                                      return_deltas=True, return_hits=True)
        err = np.max(np.abs(deltas - gold[key + "deltas"]))
        print(f"{name}: max |delta - reference| {err:.2e}")
        assert err <= DELTA_TOL, (name, err)
        assert np.array_equal(hits, gold[key + "hits"].astype(bool)), name
        assert np.array_equal(covered, hits.sum(axis=0))
        assert np.array_equal(covered / trials, gold[key + "fractions"]), name
        batch = utils.count_delta_batch(levels, counts, n_meas[: counts.shape[-2]])
        assert np.array_equal(batch, deltas), name


def test_verification_reproduces_seeded_reference_runs(gold, qp, polytopes):
    _, verification = polytopes
    levels = gold["levels"]
    for name in gold["studies"]:
        key = f"study/{name}/"
        kind, obj, kw = study_object(qp, gold, name)
        fn = verification.test_qst if kind == "state" else verification.test_qpt
        np.random.seed(int(gold[key + "seed"]))
        fractions, hits, deltas = fn(obj, levels, int(gold[key + "shots"]), int(gold[key + "trials"]), return_table=True, **kw)
        after = np.random.random()
        assert np.array_equal(fractions, gold[key + "fractions"]), name
        assert np.array_equal(hits, gold[key + "hits"].astype(bool)), name
        assert np.max(np.abs(deltas - gold[key + "deltas"])) <= DELTA_TOL, name
        assert after == float(gold[key + "random_after"]), name
        np.random.seed(int(gold[key + "seed"]))
        assert np.array_equal(fn(obj, levels, int(gold[key + "shots"]), int(gold[key + "trials"]), **kw), fractions)
    with pytest.raises(ValueError):
        verification.test_qst(qp.qobj.GHZ(1), levels, 100, 3, seed=1)  # the numpy stream is seeded by np.random.seed


# (R, K, trials, levels): every mapping and both of its edges -- wave teams (R K = 6, 64), one wavefront per trial
# (65: K not a power of two; 216), a workgroup of 256 (1 296) and of 1 024 with the frequencies in LDS (7 776, 13 824),
# a table that does not fit in LDS (21 000 entries), a one-outcome-pair table with K = 3, and a process-shaped R = D S.
SHAPES = [(3, 2, 37, 5), (16, 4, 21, 3), (13, 5, 9, 3), (27, 8, 7, 3), (2, 3, 11, 3), (81, 16, 5, 3), (243, 32, 3, 3),
          (1728, 8, 3, 2), (700, 30, 2, 2)]


@pytest.mark.parametrize("R,K,B,L", SHAPES)
def test_deltas_match_host_count_delta(eng, polytopes, R, K, B, L):
    utils, _ = polytopes
    rng = np.random.default_rng(R * 1000 + K)
    shots = rng.integers(200, 2000, size=R).astype(np.float64)
    p = rng.dirichlet(np.full(K, 0.8), size=(B, R))
    counts = np.array([[rng.multinomial(int(shots[r]), p[b, r]) for r in range(R)] for b in range(B)], dtype=np.int64)
    levels = np.array([0.0, 0.5, 0.95, 0.999, 1 - 1e-7])[:L]
    truth = np.clip(p.mean(axis=0) + 0.01, 0, 1).ravel()
    covered, deltas, hits = eng.polytope_coverage(counts, shots, levels, truth=truth, return_deltas=True, return_hits=True)
    freq = np.clip(counts / shots[:, None], EPS, 1 - EPS)
    host = np.array([[utils.count_delta(cl, f, shots) for cl in levels] for f in freq])
    err = np.max(np.abs(deltas - host))
    print(f"R K = {R * K}: max |delta - host| {err:.2e}")
    assert err <= DELTA_TOL
    margin = np.min(np.clip(freq.reshape(B, 1, -1) + deltas[:, :, None], EPS, 1 - EPS) - truth, axis=-1)
    sure = np.abs(margin + EPS) > 1e-12
    assert np.array_equal(hits[sure], (margin > -EPS)[sure])
    assert np.array_equal(covered, hits.sum(axis=0))
    # the same trials in chunks (sizes that are no multiple of the teams per wavefront): the same bits, covered accumulates
    cov2 = np.zeros(L, dtype=np.int64)
    parts_d, parts_h = [], []
    for lo, hi in ((0, 1), (1, B // 2 + 1), (B // 2 + 1, B)):
        cov2, d, h = eng.polytope_coverage(counts[lo:hi], shots, levels, truth=truth, covered=cov2, return_deltas=True,
                                           return_hits=True)
        parts_d.append(d)
        parts_h.append(h)
    assert np.array_equal(np.concatenate(parts_d), deltas) and np.array_equal(np.concatenate(parts_h), hits)
    assert np.array_equal(cov2, covered)
    # the unclipped bound of test_qpt differs only where f + delta leaves [EPS, 1 - EPS]
    cov3, hits3 = eng.polytope_coverage(counts, shots, levels, truth=truth, clip_b=False, return_hits=True)
    margin3 = np.min(freq.reshape(B, 1, -1) + deltas[:, :, None] - truth, axis=-1)
    sure3 = np.abs(margin3 + EPS) > 1e-12
    assert np.array_equal(hits3[sure3], (margin3 > -EPS)[sure3])


PUBLISHED_TRIALS = 10000
PUBLISHED_SEED = 20261016


@pytest.mark.parametrize("row", range(12))
def test_published_tables(gold, qp, polytopes, row):
    """Per entry |got - p| <= 4 sqrt(q (1 - q) (1 / T + 1 / 10000)), q = min(p, 0.999): 4 sigma of the difference of two
    independent estimates.  Per row: non-decreasing in the level (nested polytopes), and conservative."""
    _, verification = polytopes
    kind, n, shots = (int(v) for v in gold["published/rows"][row])
    levels, published = gold["published/levels"], gold["published/fractions"][row]
    T = PUBLISHED_TRIALS
    if kind == 0:
        got = verification.test_qst(qp.qobj.GHZ(n), levels, shots, T, sampler="device", seed=PUBLISHED_SEED + row)
    else:
        got = verification.test_qpt(qp.channel.depolarizing(p=0.1, n_qubits=n), levels, shots, T, sampler="device",
                                    seed=PUBLISHED_SEED + row)
    q = np.minimum(published, 0.999)
    bound = 4 * np.sqrt(q * (1 - q) * (1 / T + 1 / int(gold["published/trials"])))
    print(f"row {row} kind {kind} n {n} shots {shots}: worst (got - p) / bound = {np.max(np.abs(got - published) / bound):.2f}")
    print("  got      ", np.array2string(got, precision=4))
    print("  published", np.array2string(published, precision=4))
    assert np.all(np.abs(got - published) <= bound), (got, published)
    assert np.all(np.diff(got) >= 0)
    assert np.all(got >= levels - 4 * np.sqrt(levels * (1 - levels) / T))


def test_samplers_are_reproducible_and_chunk_invariant(qp, polytopes, monkeypatch):
    _, verification = polytopes
    levels = np.array([0.1, 0.9, 0.99])
    state = qp.qobj.GHZ(2)
    a = verification.test_qst(state, levels, 1000, 500, sampler="device", seed=5, return_table=True)
    monkeypatch.setattr(verification, "kLaunchEvaluations", 34 * 3 * 36 * 64.0)  # 64 trials per launch
    b = verification.test_qst(state, levels, 1000, 500, sampler="device", seed=5, return_table=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[1].shape == (500, 3) and np.array_equal(a[0], a[1].mean(axis=0))
    # the reference's stream in chunks: the same draws, the same state of np.random afterwards
    np.random.seed(11)
    c = verification.test_qst(state, levels, 1000, 150, return_table=True)
    after = np.random.random()
    monkeypatch.undo()
    np.random.seed(11)
    d = verification.test_qst(state, levels, 1000, 150, return_table=True)
    assert after == np.random.random()
    for x, y in zip(c, d):
        assert np.array_equal(x, y)


def test_errors_and_device_pointers(eng):
    import torch

    from quantpy_amd import _capi

    lib, h = eng.lib, eng._h
    rng = np.random.default_rng(3)
    B, R, K, L = 5, 3, 2, 4
    counts = rng.multinomial(100, [0.3, 0.7], size=(B, R)).astype(np.int64)
    shots = np.full(R, 100.0)
    levels = np.array([0.0, 0.5, 0.9, 0.99])
    truth = np.tile([0.3, 0.7], R).astype(np.float64)
    deltas = np.full((B, L), -1.0)
    hits = np.full((B, L), 7, dtype=np.uint8)
    covered = np.full(L, 100, dtype=np.int64)
    conf = np.full((B, L), -1.0)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def coverage(c=counts, b=B, r=R, k=K, n=shots, lv=levels, nl=L, t=truth, d=deltas, hh=hits, cov=covered):
        return lib.qt_polytope_coverage(h, ptr(c), b, r, k, ptr(n), ptr(lv), nl, ptr(t), 1, ptr(d), ptr(hh), ptr(cov),
                                        _capi.QT_HOST_PTR)

    def confidence(c=counts, b=B, r=R, k=K, n=shots, d=deltas, q=L, out=conf):
        return lib.qt_polytope_confidence(h, ptr(c), b, r, k, ptr(n), ptr(d), q, ptr(out), _capi.QT_HOST_PTR)

    bad_shots = [np.array([100.0, 0.0, 100.0]), np.array([100.0, -1.0, 100.0]), np.array([100.0, np.inf, 100.0]),
                 np.array([np.nan, 100.0, 100.0])]
    for call in (coverage, confidence):
        assert call(c=None) == _capi.QT_ERR_ARG
        assert call(n=None) == _capi.QT_ERR_ARG
        assert call(b=-1) == _capi.QT_ERR_ARG
        assert call(r=0) == _capi.QT_ERR_ARG
        assert call(k=0) == _capi.QT_ERR_ARG
        for s in bad_shots:
            assert call(n=s) == _capi.QT_ERR_ARG
    assert coverage(lv=None) == _capi.QT_ERR_ARG
    assert coverage(nl=0) == _capi.QT_ERR_ARG
    assert coverage(d=None, hh=None, cov=None) == _capi.QT_ERR_ARG
    assert coverage(t=None) == _capi.QT_ERR_ARG  # hits / covered need the truth
    assert confidence(d=None) == _capi.QT_ERR_ARG
    assert confidence(out=None) == _capi.QT_ERR_ARG
    assert confidence(q=0) == _capi.QT_ERR_ARG
    # nothing was launched or written by the refused calls, nor by B = 0
    assert coverage(b=0) == 0 and confidence(b=0) == 0
    assert np.all(deltas == -1.0) and np.all(hits == 7) and np.all(covered == 100) and np.all(conf == -1.0)

    assert coverage() == 0
    assert np.all(covered == 100 + hits.sum(axis=0)) and set(np.unique(hits)) <= {0, 1}
    assert coverage(t=None, hh=None, cov=None) == 0  # deltas alone need no truth
    widen = np.ascontiguousarray(deltas)
    assert confidence(d=widen) == 0

    dev = torch.device("cuda", eng.device)
    eng._dev_call()
    t_ = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    dptr = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    d_counts, d_shots, d_levels, d_truth, d_widen = t_(counts), t_(shots), t_(levels), t_(truth), t_(widen)
    d_deltas = torch.empty((B, L), dtype=torch.float64, device=dev)
    d_hits = torch.empty((B, L), dtype=torch.uint8, device=dev)
    d_cov = torch.full((L,), 100, dtype=torch.int64, device=dev)
    d_conf = torch.empty((B, L), dtype=torch.float64, device=dev)
    assert lib.qt_polytope_coverage(h, dptr(d_counts), B, R, K, dptr(d_shots), dptr(d_levels), L, dptr(d_truth), 1,
                                    dptr(d_deltas), dptr(d_hits), dptr(d_cov), _capi.QT_DEVICE_PTR) == 0
    assert lib.qt_polytope_confidence(h, dptr(d_counts), B, R, K, dptr(d_shots), dptr(d_widen), L, dptr(d_conf),
                                      _capi.QT_DEVICE_PTR) == 0
    eng.sync()
    assert np.array_equal(d_deltas.cpu().numpy(), deltas) and np.array_equal(d_hits.cpu().numpy(), hits)
    assert np.array_equal(d_cov.cpu().numpy(), covered) and np.array_equal(d_conf.cpu().numpy(), conf)
    bad = t_(np.array([100.0, 0.0, 100.0]))
    assert lib.qt_polytope_coverage(h, dptr(d_counts), B, R, K, dptr(bad), dptr(d_levels), L, dptr(d_truth), 1,
                                    dptr(d_deltas), dptr(d_hits), dptr(d_cov), _capi.QT_DEVICE_PTR) == _capi.QT_ERR_ARG


def test_unsupported_is_an_error_not_a_wrong_answer(eng):
    from quantpy_amd import _capi
    from quantpy_amd.engine import EngineError

    counts = np.zeros((1, 2, 2), dtype=np.int64)
    with pytest.raises(EngineError) as err:  # a table index that does not fit 32 bits: refused before any array is read
        eng._chk(eng.lib.qt_polytope_confidence(eng._h, counts.ctypes.data_as(ctypes.c_void_p), 1, 2**20, 2**12,
                                                counts.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p),
                                                1, counts.ctypes.data_as(ctypes.c_void_p), _capi.QT_HOST_PTR))
    assert err.value.code == _capi.QT_ERR_UNSUPPORTED
