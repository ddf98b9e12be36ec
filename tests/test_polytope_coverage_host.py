"""quantpy_amd.tomography.polytopes on the host: the module layout, the reference's signatures, and the host functions
count_confidence / count_delta against tests/golden/polytope_coverage.npz (make_golden_polytope_coverage.py: the
reference's numbers, an extended-precision evaluation of the same formula, and seeded runs of the reference's
test_qst / test_qpt).  Nothing here needs a GPU: POVM tensors above one qubit are assembled with np.kron, which is what
the device assembly reproduces bit for bit.

The module is imported, never the names test_qst / test_qpt: pytest would collect them."""
import inspect

import numpy as np
import pytest
from conftest import load_golden

from quantpy_amd.tomography import interval
from quantpy_amd.tomography.polytopes import utils, verification

EPS = 1e-15
DELTA_TOL = 2.5e-10  # two bisections whose comparisons differ only within rounding of the level: bracket width 1.16e-10 x 2


@pytest.fixture(scope="module")
def gold():
    return load_golden("polytope_coverage")


def kron_power(table, n):
    out = np.asarray(table)
    for _ in range(n - 1):
        out = np.kron(out, table)
    return out


def study_setup(gold, name):
    """(probas, shots, truth, clip_b) of a stored study, formed on the host."""
    import quantpy_amd as qp
    from quantpy_amd.measurements import generate_measurement_matrix

    key = f"study/{name}/"
    n, shots = int(gold[key + "n_qubits"]), int(gold[key + "shots"])
    povm = kron_power(generate_measurement_matrix("proj-set", 1), n)
    if key + "rho" in gold.files:
        return (*verification.qst_setup(qp.Qobj(gold[key + "rho"]), shots, povm=povm), True)
    inputs = []
    for bloch in np.squeeze(kron_power(generate_measurement_matrix(str(gold[key + "input_states"]), 1), n)):
        state = qp.Qobj(bloch)
        state /= state.trace()
        inputs.append(state)
    channel = qp.channel.depolarizing(p=float(gold[key + "depolarizing_p"]), n_qubits=n)
    return (*verification.qpt_setup(channel, shots, input_states=inputs, povm=povm), False)


def test_utils_are_the_interval_functions():
    assert utils.count_confidence is interval.count_confidence
    assert utils.count_delta is interval.count_delta
    assert callable(utils.count_delta_batch)


def test_reference_signatures():
    qst = inspect.signature(verification.test_qst)
    qpt = inspect.signature(verification.test_qpt)
    positional = lambda sig: [(p.name, p.default) for p in sig.parameters.values()  # noqa: E731
                              if p.kind == p.POSITIONAL_OR_KEYWORD]
    empty = inspect.Parameter.empty
    assert positional(qst) == [("state", empty), ("conf_levels", empty), ("n_measurements", 1000), ("n_trials", 1000)]
    assert positional(qpt) == [("channel", empty), ("conf_levels", empty), ("n_measurements", 1000), ("n_trials", 1000),
                               ("input_states", "sic")]
    for sig in (qst, qpt):
        extra = {p.name: p.default for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY}
        assert extra == {"sampler": "numpy", "seed": None, "return_table": False}
    assert list(inspect.signature(utils.count_confidence).parameters) == ["delta", "frequencies", "n_measurements"]
    assert list(inspect.signature(utils.count_delta).parameters) == ["target_cl", "frequencies", "n_measurements"]


def test_chunk_trials_bounds():
    assert verification.chunk_trials(10000, 6, 18) == 10000
    big = verification.chunk_trials(10000, 13824, 18)
    assert 1 <= big < 10000 and big * 13824 * 8 <= verification.kChunkBytes
    assert big * 18 * 34 * 13824 <= verification.kLaunchEvaluations
    assert verification.chunk_trials(5, 10**9, 18) == 1


def test_count_confidence_formula_cases(gold):
    for name in gold["formula_groups"]:
        key = f"formula/{name}/"
        counts, shots, deltas = gold[key + "counts"], gold[key + "shots"], gold[key + "deltas"]
        ext = gold[key + "ext_hi"].astype(np.longdouble) + gold[key + "ext_lo"].astype(np.longdouble)
        ref, e_ref = gold[key + "ref"], float(gold[key + "e_ref"])
        tol = 4 * e_ref + 4e-16
        for t in range(counts.shape[0]):
            freq = np.clip(counts[t] / shots[:, None], EPS, 1 - EPS)
            got = np.array([utils.count_confidence(d, freq, shots) for d in deltas[t]])
            err = np.max(np.abs(got.astype(np.longdouble) - ext[t]))
            print(f"{name} table {t}: e_ref {e_ref:.2e} host error {float(err):.2e}")
            assert err <= tol, (name, t, float(err), tol)
            assert np.array_equal(got[ref[t] == 0.0], ref[t][ref[t] == 0.0])
            assert np.array_equal(got[ref[t] == 1.0], ref[t][ref[t] == 1.0])


def test_seeded_studies_on_the_host(gold):
    levels = gold["levels"]
    for name in gold["studies"]:
        key = f"study/{name}/"
        probas, shots, truth, clip_b = study_setup(gold, name)
        counts = gold[key + "counts"]
        trials = counts.shape[0]
        freq = np.clip(counts.reshape(trials, *probas.shape) / shots[:, None], EPS, 1 - EPS)
        deltas = np.array([[utils.count_delta(cl, f, shots) for cl in levels] for f in freq])
        err = np.max(np.abs(deltas - gold[key + "deltas"]))
        print(f"{name}: max |delta - reference| {err:.2e}")
        assert err <= DELTA_TOL, (name, err)
        bound = freq.reshape(trials, 1, -1) + deltas[:, :, None]
        if clip_b:
            bound = np.clip(bound, EPS, 1 - EPS)
        margin = np.min(bound - truth, axis=-1)
        assert np.min(np.abs(margin + EPS)) >= 1e-8 - DELTA_TOL  # the fixture's asserted margin, less the delta tolerance
        hits = margin > -EPS
        assert np.array_equal(hits, gold[key + "hits"].astype(bool)), name
        assert np.array_equal(hits.sum(axis=0) / trials, gold[key + "fractions"]), name


def test_published_tables_shape(gold):
    assert gold["published/fractions"].shape == (12, 18) and gold["published/rows"].shape == (12, 3)
    assert np.allclose(gold["published/levels"], np.concatenate((np.arange(0.1, 0.9, 0.1), np.arange(0.9, 1, 0.01))))
    assert np.all(gold["published/fractions"] >= gold["published/levels"])
