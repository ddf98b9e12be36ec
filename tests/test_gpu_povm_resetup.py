"""GPU: qt_set_povm / qt_set_povm_product more than once on one engine -- registrations of different kinds in turn
(n = 1, 2, 3: product and plain, equal and unequal shots, six- and four-row one-qubit tables), a good registration after
a failed one (n = 2), and a qt_povm_kron call between a registration and the dense operands built on demand from it
(n = 4).  What an engine computes after a registration depends on that registration alone: every result is compared bit
for bit with a fresh engine that has seen nothing else."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _states(n, count, seed):
    """`count` full-rank density matrices, 0.8 |psi><psi| + 0.2 I / d."""
    rng = np.random.default_rng(seed)
    d = 2**n
    psi = rng.normal(size=(count, d)) + 1j * rng.normal(size=(count, d))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    return 0.8 * psi[:, :, None] * psi[:, None, :].conj() + 0.2 * np.eye(d) / d


def _counts(rng, probs, shots, trials):
    """(trials, S, K) multinomial counts: setting s of every trial gets shots[s] of them."""
    p = np.clip(probs, 0.0, None)
    p /= p.sum(axis=-1, keepdims=True)
    return np.stack([[rng.multinomial(int(ns), ps) for ns, ps in zip(shots, p)] for _ in range(trials)]).astype(np.int64)


def _results(eng, bloch, counts):
    rho, info = eng.mle(counts, return_info=True)
    spec = eng.mle_specialised  # (of the `mle` just made)
    return {"left_inverse": eng.left_inverse(), "born_probs": eng.born_probs(bloch), "lin": eng.lin(counts), "mle": rho,
            "nit": info["nit"], "nfev": info["nfev"], "fun": info["fun"], "status": info["status"],
            "paired_tables": np.int64(eng.paired_tables), "mle_specialised": np.bool_(spec)}


def _assert_same(got, want, where):
    assert got.keys() == want.keys()
    for key in want:
        assert np.array_equal(got[key], want[key]), (where, key)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_registrations_of_different_kinds_in_turn(n):
    import quantpy_amd as qp

    proj = qp.generate_measurement_matrix("proj-set", n)
    sic = qp.generate_measurement_matrix("sic", n)
    s = proj.shape[0]
    equal, unequal = np.full(s, 1000), 1000 + 40 * (np.arange(s) % 3)
    turns = [("proj-set", proj, equal), ("plain array", np.asarray(proj), equal), ("unequal shots", proj, unequal),
             ("sic", sic, np.full(1, 1000)), ("proj-set", proj, equal)]
    assert proj.valid_factor() is not None and not hasattr(turns[1][1], "valid_factor")
    states = _states(n, 3, 100 + n)
    eng = qp.Engine(n)
    for turn, (name, povm, shots) in enumerate(turns):
        fresh = qp.Engine(n)
        for e in (eng, fresh):
            e.set_povm(povm, shots)
        bloch = fresh.bloch_from_matrix(states)
        counts = _counts(np.random.default_rng(7 * n + turn), fresh.born_probs(bloch)[0], shots, 5)
        want = _results(fresh, bloch, counts)
        _assert_same(_results(eng, bloch, counts), want, (turn, name))
        # the turns are of the kinds they are meant to be
        product = name != "plain array"
        assert fresh.product == product
        assert int(want["paired_tables"]) == (3 if product and name != "sic" else 0), name
        assert bool(want["mle_specialised"]) == (name == "proj-set"), name
        fresh.close()
    eng.close()


def test_good_registration_after_a_failed_one():
    """A six-row one-qubit table without a Z part is not informationally complete: qt_set_povm_product fails with
    QT_ERR_SINGULAR after it has reset the handle, and leaves it without a POVM; the registration of 'proj-set' that
    follows behaves like the first on a fresh engine."""
    import quantpy_amd as qp
    from quantpy_amd import _capi

    n = 2
    proj = qp.generate_measurement_matrix("proj-set", n)
    xyx = np.array([[[1, 1, 0, 0], [1, -1, 0, 0]], [[1, 0, 1, 0], [1, 0, -1, 0]], [[1, 1, 0, 0], [1, -1, 0, 0]]]) / 2
    flat = qp.generate_measurement_matrix(xyx, n)
    assert flat.shape == proj.shape and flat.valid_factor() is not None
    shots = np.full(proj.shape[0], 1000)
    eng, fresh = qp.Engine(n), qp.Engine(n)
    eng.set_povm(proj, shots)
    fresh.set_povm(proj, shots)
    bloch = fresh.bloch_from_matrix(_states(n, 3, 41))
    counts = _counts(np.random.default_rng(43), fresh.born_probs(bloch)[0], shots, 5)
    with pytest.raises(qp.EngineError) as ei:
        eng.set_povm(flat, shots)
    assert ei.value.code == _capi.QT_ERR_SINGULAR
    with pytest.raises(qp.EngineError) as ei:
        eng.lin(counts)
    assert ei.value.code == _capi.QT_ERR_STATE
    eng.set_povm(proj, shots)
    _assert_same(_results(eng, bloch, counts), _results(fresh, bloch, counts), "after the failed registration")
    eng.close()
    fresh.close()


def test_kron_cache_is_not_the_povm():
    """n = 4 builds a product POVM's dense operands on demand, from the registered one-qubit factor: a qt_povm_kron call
    with a table of another shape in between (here the smaller 'sic' table after the six-row 'proj-set') changes nothing.
    (The dense tensor used to be assembled with the shape that call left in the handle's digit cache.)"""
    import quantpy_amd as qp

    n = 4
    proj = qp.generate_measurement_matrix("proj-set", n)
    sic1 = qp.generate_measurement_matrix("sic", 1)[0]
    assert proj.shape == (81, 16, 256) and sic1.shape == (4, 4)
    shots = 1000 + 40 * (np.arange(81) % 3)
    eng, fresh = qp.Engine(n), qp.Engine(n)
    for e in (eng, fresh):
        e.set_povm(proj, shots)
    assert eng.product and fresh.product
    kron = eng.povm_kron(sic1[None])
    assert kron.shape == (1, 256, 256)
    counts = _counts(np.random.default_rng(47), np.full((81, 16), 1 / 16), shots, 2)
    assert np.array_equal(eng.left_inverse(), fresh.left_inverse())
    assert np.array_equal(eng.lin(counts), fresh.lin(counts))
    eng.close()
    fresh.close()
