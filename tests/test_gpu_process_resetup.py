"""GPU: qt_process_setup more than once on one engine -- set-ups of different kinds in turn (n = 2: the dense form with
and without the Kronecker factors and the permuted operand of k_lifp16) and a good set-up after a failed one (n = 1: the
dense branch, n = 3: the factored one).  What an engine computes after a set-up depends on that set-up alone: every
result is compared bit for bit with a fresh engine that has seen nothing else."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _input_states(n):
    from quantpy_amd.tomography.process import _generate_input_states

    return np.stack([np.asarray(s.matrix, dtype=np.complex128) for s in _generate_input_states("proj4", n)])


def _setup(eng, povm, shots, states):
    eng.set_povm(povm, shots)
    eng.process_setup(states)


def test_n2_setups_of_different_kinds_in_turn():
    """A: 'proj-set' (M = 36: factors and permuted operand), B: the five-outcome one-qubit POVM of
    test_lifp_batched_ragged_povm_and_nan_isolation (M = 25: dense form only), A again.  Batches of 3 and 260 take both
    sides of the B >= 256 choice of the dense-operator path."""
    import quantpy_amd as qp
    from quantpy_amd import _capi

    states = _input_states(2)
    sic = qp.generate_measurement_matrix("sic", 1)[0]
    five = np.vstack([sic[:1] / 2, sic[:1] / 2, sic[1:]])
    povms = {"A": qp.generate_measurement_matrix("proj-set", 2), "B": qp.generate_measurement_matrix(five, 2)}
    assert np.asarray(povms["A"]).shape == (9, 4, 16) and np.asarray(povms["B"]).shape == (1, 25, 16)
    rng = np.random.default_rng(23)
    counts = {"A": rng.multinomial(4000, np.full(4, 0.25), size=(260, 16, 9)).astype(np.int64),
              "B": rng.multinomial(4000, np.full(25, 0.04), size=(260, 16, 1)).astype(np.int64)}
    eng = qp.Engine(2)
    for kind in "ABA":
        fresh = qp.Engine(2)
        for e in (eng, fresh):
            _setup(e, povms[kind], 4000, states)
        for cptp in (False, True):
            for b in (3, 260):
                assert np.array_equal(eng.lifp(counts[kind][:b], cptp=cptp), fresh.lifp(counts[kind][:b], cptp=cptp)), (kind, cptp, b)
        if kind == "A":
            for got, want in zip(eng.process_factors(), fresh.process_factors()):
                assert np.array_equal(got, want)
        else:
            with pytest.raises(qp.EngineError) as ei:
                eng.process_factors()
            assert ei.value.code == _capi.QT_ERR_UNSUPPORTED
            oper, inv = eng.process_operators()
            assert oper.shape == (400, 256) and np.isfinite(oper).all() and np.isfinite(inv).all()
        fresh.close()
    eng.close()


@pytest.mark.parametrize("n", [1, 3])
def test_good_setup_after_a_failed_one(n):
    """D copies of one input state do not span the operator space: the set-up fails with QT_ERR_SINGULAR and leaves the
    engine without one; the set-up with the real input states that follows behaves like the first on a fresh engine."""
    import quantpy_amd as qp
    from quantpy_amd import _capi

    states = _input_states(n)
    povm = qp.generate_measurement_matrix("proj-set", n)
    rng = np.random.default_rng(29 + n)
    counts = rng.multinomial(1000, np.full(2**n, 0.5**n), size=(2, 4**n, 3**n)).astype(np.int64)
    eng, fresh = qp.Engine(n), qp.Engine(n)
    eng.set_povm(povm, 1000)
    with pytest.raises(qp.EngineError) as ei:
        eng.process_setup(np.stack([states[0]] * 4**n))
    assert ei.value.code == _capi.QT_ERR_SINGULAR
    with pytest.raises(qp.EngineError) as ei:
        eng.lifp(counts)
    assert ei.value.code == _capi.QT_ERR_STATE
    for e in (eng, fresh):
        _setup(e, povm, 1000, states)
    for cptp in (False, True):
        assert np.array_equal(eng.lifp(counts, cptp=cptp), fresh.lifp(counts, cptp=cptp)), cptp
    eng.close()
    fresh.close()
