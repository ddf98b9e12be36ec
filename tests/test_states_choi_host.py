"""Host: the weights W of the 'states' process estimator reproduce the einsum assembly they replace, the three C entries
behind the estimator are bound with the header's argument lists, and get_CL_list_channel_boot_states refuses bad arguments
before anything touches the GPU."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

import quantpy_amd as qp
from quantpy_amd import _capi, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def einsum_assembly(tmg, outs):
    """The assembly of point_estimate_batch(method='states') as it stood before the weights: sum_e unit_e (x) image_e."""
    ins = np.stack([np.asarray(s.matrix, dtype=np.complex128) for s in tmg.input_basis.elements])
    coeff = tmg._decomposed_single_entries
    units = np.einsum("es,sab->eab", coeff, ins)
    images = np.einsum("es,bsac->beac", coeff, outs)
    dim = ins.shape[1]
    return np.einsum("eij,bekl->bikjl", units, images).reshape(outs.shape[0], dim * dim, dim * dim)


def weights_assembly(w, outs):
    """C_b[(i,k),(j,l)] = sum_s W[(i,j),s] rho_b,s[k,l]: one D x D by D x D product per trial and a permutation."""
    b, dd, d = outs.shape[:3]
    prod = w[None] @ outs.reshape(b, dd, dd)
    return prod.reshape(b, d, d, d, d).transpose(0, 1, 3, 2, 4).reshape(b, dd, dd)


def random_hermitian_states(rng, b, dd, d):
    g = rng.standard_normal((b, dd, d, d)) + 1j * rng.standard_normal((b, dd, d, d))
    return (g + np.conj(np.swapaxes(g, -1, -2))) / 2  # Hermitian, not PSD, distinct per trial


def product_inputs(name, n):
    """The input states the named POVM gives at n qubits, as a list: the n-fold products of its one-qubit states (the
    named form tensors the table up on the GPU; this test has none)."""
    from quantpy_amd.tomography.process import _generate_input_states

    one = _generate_input_states(name, 1)
    states = one
    for _ in range(n - 1):
        states = [a.kron(b) for a in states for b in one]
    return states


@pytest.mark.parametrize("inputs", ["proj4", "sic"])
@pytest.mark.parametrize("n", [1, 2])
def test_weights_reproduce_the_einsum_assembly(n, inputs):
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.3, n), input_states=product_inputs(inputs, n))
    d, dd = 2**n, 4**n
    w = tmg._states_weights()
    assert w.shape == (dd, dd) and w.dtype == np.complex128 and w.flags.c_contiguous
    outs = random_hermitian_states(np.random.default_rng(11 + n), 5, dd, d)
    old, new = einsum_assembly(tmg, outs), weights_assembly(w, outs)
    # both sum D products per entry: 8 D eps on the sum of the products' moduli, per entry, its maximum taken
    bound = 8 * dd * EPS * (np.abs(w)[None] @ np.abs(outs.reshape(5, dd, dd))).max()
    err = np.abs(new - old).max()
    print(f"n={n} {inputs}: |W form - einsum form| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


_C_TYPES = {"int": ctypes.c_int, "double": ctypes.c_double}


@pytest.mark.parametrize("name", ["qt_states_choi_batch", "qt_states_choi_dist_group_batch", "qt_choi_is_cptp_batch"])
def test_entries_are_bound_as_declared(name):
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name
    declared = []
    for arg in m.group(1).split(","):
        kind = arg.strip().rsplit(" ", 1)[0]
        declared.append(ctypes.c_void_p if kind.endswith("*") else _C_TYPES[kind])
    assert name in _capi.SIGNATURES
    assert _capi.SIGNATURES[name] == (ctypes.c_int, declared)


def test_entry_argument_lists():
    assert len(_capi.SIGNATURES["qt_states_choi_batch"][1]) == 9
    assert len(_capi.SIGNATURES["qt_states_choi_dist_group_batch"][1]) == 12
    assert len(_capi.SIGNATURES["qt_choi_is_cptp_batch"][1]) == 6


def test_study_signature():
    params = list(inspect.signature(metrics.get_CL_list_channel_boot_states).parameters.values())
    assert [p.name for p in params] == [
        "channel", "n_iter", "n_points", "n_measurements", "method", "povm", "input_states", "cptp", "states_physical",
        "states_init", "states_est_method", "states_est_method_boot", "sampler", "seed", "chunk", "return_details", "dst"]
    assert {p.name: p.default for p in params[1:]} == dict(
        n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set", input_states="proj4", cptp=True,
        states_physical=True, states_init="lin", states_est_method="lin", states_est_method_boot="lin", sampler="device",
        seed=None, chunk=None, return_details=False, dst="hs")
    assert all(p.kind is p.KEYWORD_ONLY for p in params[-5:])


def test_study_refuses_bad_arguments_before_any_device_work():
    had_torch = "torch" in sys.modules
    study = metrics.get_CL_list_channel_boot_states
    for bad in ("pgdb", "lifp", None):
        with pytest.raises(NotImplementedError, match="states_est_method_boot"):
            study(None, states_est_method_boot=bad)
    with pytest.raises(ValueError, match="dst"):
        study(None, dst="bures")
    for kw in (dict(n_points=0), dict(n_points=-2), dict(n_iter=0)):
        with pytest.raises(ValueError, match="positive"):
            study(None, **kw)
    with pytest.raises(ValueError, match="sampler"):
        study(None, sampler="cupy")
    assert had_torch or "torch" not in sys.modules


def test_the_old_refusal_stays_and_the_docstring_names_the_study():
    with pytest.raises(NotImplementedError, match="boot") as err:
        metrics.get_CL_list_channel(None, interval="boot")
    assert "get_CL_list_channel_boot_states" not in str(err.value)  # the refusal's text is untouched
    assert "get_CL_list_channel_boot_states" in metrics.get_CL_list_channel.__doc__
