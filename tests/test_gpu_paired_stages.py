"""GPU: the contraction stages of paired one-qubit tables (six rows, rows 2a and 2a+1 exactly zero outside columns 0
and a+1: 'proj-set', 'proj' and their pseudo-inverses) against the dense-table stages of the same launch
(QT_OPT_PAIRED_STAGES 1 / 0).  The paired stages drop terms fma(0, x, acc) and keep the rest in their order, so
"equal" below is np.array_equal on finite outputs: nothing but the sign of a zero may differ."""
import numpy as np
import pytest
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _ginibre(rng, d, rank=None):
    g = rng.standard_normal((d, rank or d)) + 1j * rng.standard_normal((d, rank or d))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _estimates(eng, capi, counts, x, centre):
    """Everything the factorised stages feed: 'lin', the NLL, the MLE through both launch forms, the one-pass distance."""
    out = {}
    rho, bloch = eng.lin(counts, physical=False, return_bloch=True)
    out["lin_raw"], out["lin_bloch"], out["lin"] = rho, bloch, eng.lin(counts)
    out["nll_f"], out["nll_g"] = eng.nll(x, counts)
    try:
        for path, waves in (("fused", 1024), ("split", 0)):
            eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, waves)
            for init in ("lin", "mixed"):
                rho, info = eng.mle(counts, init=init, return_info=True)
                out[f"mle_{path}_{init}_rho"] = rho
                for k, v in info.items():
                    out[f"mle_{path}_{init}_{k}"] = v
    finally:
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    out["mle_dist"] = eng.mle_dist(counts, centre)
    return out


def _on_off(eng, capi, fn):
    """fn() with the paired stages on, then forced off."""
    try:
        eng.set_option(capi.QT_OPT_PAIRED_STAGES, 1)
        on = fn()
        eng.set_option(capi.QT_OPT_PAIRED_STAGES, 0)
        off = fn()
    finally:
        eng.set_option(capi.QT_OPT_PAIRED_STAGES, 1)
    return on, off


def _assert_same_bits(on, off, what):
    assert on.keys() == off.keys()
    for k in on:
        a, b = np.asarray(on[k]), np.asarray(off[k])
        assert np.isfinite(a).all() and np.isfinite(b).all(), (what, k)
        assert np.array_equal(a, b), (what, k, np.abs(a - b).max())


def _trial_sets(oracle, a_dense, n, rng, seed):
    """(tag, counts (9, S, K)): a Ginibre state at 400 shots per setting (clipped trials, BFGS iterates) and at 1e5
    (the headline regime); at n = 3 a rank-1 state as well."""
    d = 2**n
    np.random.seed(seed)
    states = [("ginibre", _ginibre(rng, d))] + ([("rank1", _ginibre(rng, d, 1))] if n == 3 else [])
    sets = []
    for tag, rho in states:
        bloch = oracle.bloch_from_matrix(rho)
        for shots in (400, 100000):
            sets.append((f"{tag}-{shots}", np.stack([oracle.sample_counts(a_dense, bloch, shots) for _ in range(9)])))
    return sets, states[0][1]


@pytest.mark.parametrize("name", ["proj-set", "proj"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_paired_stages_give_the_bits_of_the_dense_table_stages(qp, oracle, n, name):
    from quantpy_amd import _capi

    rng = np.random.default_rng(100 + n)
    d = 2**n
    a = qp.generate_measurement_matrix(name, n)
    eng = qp.get_engine(n)
    sets, rho0 = _trial_sets(oracle, np.array(a), n, rng, 11 + n)
    x = np.stack([oracle.matrix_to_tril_vec(rho0) + 0.03 * rng.standard_normal(d * d) for _ in range(9)])
    for tag, counts in sets:  # nine trials: not a multiple of the trials per workgroup, the padding lanes run
        eng.set_povm(a, counts[0].sum(-1))
        assert eng.product and eng.paired_tables & 1
        if name == "proj-set":  # c = 1/2: T^T T and its inverse are exact, the device's pseudo-inverse is sparse
            assert eng.paired_tables == 3
        on, off = _on_off(eng, _capi, lambda: _estimates(eng, _capi, counts, x, rho0))
        _assert_same_bits(on, off, (n, name, tag))


def _perturbed_proj_set():
    t = np.array([[[1, 1, 0, 0], [1, -1, 0, 0]], [[1, 0, 1, 0], [1, 0, -1, 0]], [[1, 0, 0, 1], [1, 0, 0, -1]]]) / 2
    t[1, 0, 3] = 1e-300  # a structural zero that is not one
    return t


def _unequal_pairs():
    t = np.array([[[1, 1, 0, 0], [1, -1, 0, 0]], [[1, 0, 1, 0], [1, 0, -1, 0]], [[1, 0, 0, 1], [1, 0, 0, -1]]]) / 2
    t[:, 0] *= 0.9  # free coefficients (u_r, v_r) per row: no +- symmetry inside a pair
    t[:, 1] *= 1.1
    return t


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("povm", ["sic", "proj4", "proj-set-1e-300", "unequal-pairs"])
def test_what_is_paired_and_agreement_with_the_dense_operand_path(qp, oracle, n, povm):
    """Tables that must not be taken for paired report 0 and run the dense-table stages; a six-row table with
    unequal coefficients is paired.  Either way the factorised path agrees with the dense-operand path (a plain
    ndarray) to the bounds of test_gpu_product.py: 1e-12 on the value, 1e-10 on the gradient."""
    from quantpy_amd import _capi

    rng = np.random.default_rng(7 * n + len(povm))
    d = 2**n
    table = {"proj-set-1e-300": _perturbed_proj_set, "unequal-pairs": _unequal_pairs}.get(povm, lambda: povm)()
    a_prod = qp.generate_measurement_matrix(table, n)
    a_dense = np.array(a_prod)
    # counts are only integers here: drawn from a normalised POVM of the same shape ('proj4' does not sum to 1)
    a_draw = np.array(qp.generate_measurement_matrix("sic" if isinstance(table, str) else "proj-set", n))
    rho = _ginibre(rng, d)
    np.random.seed(5)
    counts = np.stack([oracle.sample_counts(a_draw, oracle.bloch_from_matrix(rho), 400) for _ in range(9)])
    x = np.stack([oracle.matrix_to_tril_vec(rho) + 0.03 * rng.standard_normal(d * d) for _ in range(9)])
    eng = qp.get_engine(n)
    eng.set_povm(a_dense, counts[0].sum(-1))
    assert not eng.product and eng.paired_tables == 0
    f_d, g_d = eng.nll(x, counts)
    _, bl_d = eng.lin(counts, physical=False, return_bloch=True)
    eng.set_povm(a_prod, counts[0].sum(-1))
    assert eng.product
    if povm == "unequal-pairs":
        assert eng.paired_tables & 1
    else:
        assert eng.paired_tables == 0
    on, off = _on_off(eng, _capi, lambda: _estimates(eng, _capi, counts, x, rho))
    _assert_same_bits(on, off, (n, povm))
    assert np.abs(on["nll_f"] - f_d).max() < 1e-12 and np.abs(on["nll_g"] - g_d).max() < 1e-10
    assert np.abs(on["lin_bloch"] - bl_d).max() < 1e-12


def test_unequal_shots_pair_the_nll_and_keep_the_dense_inverse(qp, oracle):
    """Shots (100, 2000, 30000): the row weights differ, so 'lin' multiplies by the dense left inverse while the NLL
    still factorises and takes the paired stages of T."""
    from quantpy_amd import _capi

    g = load_golden("counts_lin")
    counts = g["L0_counts"]  # n = 1
    eng = qp.get_engine(1)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", 1), counts.sum(-1))
    assert eng.product and eng.paired_tables == 3
    rng = np.random.default_rng(4)
    x = oracle.matrix_to_tril_vec(_ginibre(rng, 2)) + 0.03 * rng.standard_normal(4)

    def run():
        rho, info = eng.mle(counts, return_info=True)
        f, gr = eng.nll(x, counts)
        return dict(lin=eng.lin(counts), nll_f=f, nll_g=gr, mle=rho, **info)

    on, off = _on_off(eng, _capi, run)
    _assert_same_bits(on, off, "L0")
    assert np.abs(on["lin"] - g["L0_lin"]).max() < 1e-12
    fo, go = oracle.NllProblem(counts, oracle.measurement_matrix("proj-set", 1)).nll_and_grad(x)
    assert abs(on["nll_f"] - fo) < 1e-12 and np.abs(on["nll_g"] - go).max() < 1e-10


def test_metropolis_chain_value_only_evaluations(qp, oracle):
    """k_mhmc_state evaluates the NLL without its gradient: three chains of eight steps at n = 2."""
    from quantpy_amd import _capi

    n, d = 2, 4
    rng = np.random.default_rng(21)
    a = qp.generate_measurement_matrix("proj-set", n)
    states = [_ginibre(rng, d) for _ in range(3)]
    np.random.seed(22)
    counts = np.stack([oracle.sample_counts(np.array(a), oracle.bloch_from_matrix(s), 1000) for s in states])
    eng = qp.get_engine(n)
    eng.set_povm(a, counts[0].sum(-1))
    assert eng.paired_tables == 3
    x0 = np.stack([oracle.matrix_to_tril_vec(s) for s in states])
    deltas, uniforms = rng.standard_normal((3, 8, d * d)), rng.random((3, 8))
    on, off = _on_off(eng, _capi, lambda: dict(zip(("chain", "acc"), eng.mhmc_state(counts, x0, deltas, uniforms, 0.05))))
    _assert_same_bits(on, off, "mhmc")
