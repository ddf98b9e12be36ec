"""No GPU: the surface of the chain coverage study of three-qubit channels -- the two C entries
(qt_mhmc_process_large_hits, qt_mhmc_process_large_metric_hits) as the header declares them and _capi binds them, the
slice option, and the argument handling of metrics.get_CL_list_channel_mhmc_large."""
import ctypes
import inspect
import os
import re
import sys

import pytest

from quantpy_amd import _capi, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = (("qt_mhmc_process_large_hits", "qt_mhmc_process_hits"),
         ("qt_mhmc_process_large_metric_hits", "qt_mhmc_process_metric_hits"))
_CTYPES = {"int": ctypes.c_int, "uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}


def _header():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        return fh.read()


def _declaration(header, name):
    m = re.search(r"^int " + name + r"\((.*?)\);", header, re.S | re.M)
    assert m, name
    args = [" ".join(a.split()) for a in m.group(1).replace("\n", " ").split(",")]
    return [(a.rsplit(" ", 1)[0].rstrip("* ") + ("*" if "*" in a else ""), a.rsplit(" ", 1)[1].lstrip("*")) for a in args]


def test_capi_declares_the_two_entries_as_the_header_states_them():
    header = _header()
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for large, sibling in PAIRS:
        decl = _declaration(header, large)
        restype, argtypes = _capi.SIGNATURES[large]
        assert restype is ctypes.c_int and hasattr(lib, large)
        assert argtypes == [ctypes.c_void_p if t.endswith("*") else _CTYPES[t] for t, _ in decl], (large, decl)
        # the argument lists of the n <= 2 entries
        assert decl == _declaration(header, sibling)
        assert _capi.SIGNATURES[large] == _capi.SIGNATURES[sibling]
    names = [a for _, a in _declaration(header, "qt_mhmc_process_large_metric_hits")]
    assert names == ["h", "metric", "counts", "C", "centres", "choi_init", "thresholds", "seed", "first_chain", "burn_steps",
                     "n_points", "thinning", "step", "hits", "accepted", "dist", "flags"]


def test_slice_option_is_number_seven_in_header_and_capi():
    assert _capi.QT_OPT_MHMC_PROCESS_SLICE == 7
    assert re.search(r"QT_OPT_MHMC_PROCESS_SLICE\s*=\s*7\b", _header())


def test_study_has_the_signature_of_the_smaller_study():
    small = inspect.signature(metrics.get_CL_list_channel_mhmc)
    large = inspect.signature(metrics.get_CL_list_channel_mhmc_large)
    assert large == small
    assert [p.name for p in large.parameters.values() if p.kind is p.KEYWORD_ONLY] == ["sampler", "seed", "return_details",
                                                                                         "dst"]
    assert large.parameters["step"].default == 0.01 and large.parameters["burn_steps"].default == 1000


def test_argument_errors_before_any_gpu_use():
    had_torch = "torch" in sys.modules
    fn = metrics.get_CL_list_channel_mhmc_large  # (the channel is never looked at: these come in front of everything else)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_iter=0)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_points=0)
    with pytest.raises(ValueError, match="sampler"):
        fn(None, sampler="sobol")
    with pytest.raises(ValueError, match="thinning"):
        fn(None, thinning=0)
    with pytest.raises(ValueError, match="burn_steps"):
        fn(None, burn_steps=-1)
    with pytest.raises(ValueError, match="2\\^32"):
        fn(None, n_points=2**20, thinning=2**12)
    with pytest.raises(ValueError, match="dst"):
        fn(None, dst="bures")
    assert had_torch or "torch" not in sys.modules


def test_sizes_are_refused_before_the_engine_is_touched(monkeypatch):
    """Four qubits by the new name, three by the old one with its text: both before the tomograph is built."""
    import quantpy_amd as qp
    from quantpy_amd.tomography.process import ProcessTomograph

    def no_tomograph(*a, **k):
        raise AssertionError("the refusal must come before the tomograph is built")

    monkeypatch.setattr(ProcessTomograph, "__init__", no_tomograph)
    monkeypatch.setattr(ProcessTomograph, "_engine", no_tomograph)
    with pytest.raises(NotImplementedError, match="one and two qubits"):
        metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1)
    with pytest.raises(NotImplementedError, match="one to three qubits"):
        metrics.get_CL_list_channel_mhmc_large(qp.channel.depolarizing(0.1, 4), n_iter=2, n_points=3, burn_steps=1)
    with pytest.raises(AssertionError, match="before the tomograph"):  # three qubits go on to the study
        metrics.get_CL_list_channel_mhmc_large(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1)


def test_docstrings_say_which_name_serves_which_size():
    assert "get_CL_list_channel_mhmc_large" in metrics.get_CL_list_channel_mhmc.__doc__
    doc = metrics.get_CL_list_channel_mhmc_large.__doc__
    assert "get_CL_list_channel_mhmc" in doc and "step" in doc and "1e-5" in doc
