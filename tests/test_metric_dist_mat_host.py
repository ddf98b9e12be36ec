"""Host: the surface of the trace distance / infidelity up to dim 64 (qt_metric_dist_mat) without a GPU -- the C entry is
declared behind its sibling and exported, the binding has its ten arguments, the rules a caller relies on stand where the
entry is declared, and the intervals of a three-qubit channel may ask the engine for these distances."""
import ctypes
import os
import re

from quantpy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qt_metric_dist_mat"


def _header():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        return fh.read()


def test_entry_is_declared_exported_and_bound():
    header = _header()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/qtomo.h"
    assert NAME in _capi.SIGNATURES and len(_capi.SIGNATURES[NAME][1]) == m.group(1).count(",") + 1 == 10
    assert _capi.SIGNATURES[NAME] == _capi.SIGNATURES["qt_metric_dist_dim"]
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    # declared behind the sibling, whose arguments it takes
    assert header.index("int qt_metric_dist_dim(") < m.start()
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["h", "metric", "dim", "rho", "B", "centres", "G", "g0", "dist", "flags"]


def test_header_comment_states_the_rules():
    header = _header()
    at = header.index("int " + NAME + "(")
    doc = header[header.rindex("/*", 0, at):at]
    for word in ("geometry.py:23-38", ":41-56", "HERMITIAN", "1e-15", "NaN", "QT_ERR_UNSUPPORTED", "QT_ERR_ARG",
                 "dim = 64", "2, 4, 8, 16, 32, 64", "SECOND", "B == 0 returns 0"):
        assert word in doc, word


def test_choi_intervals_may_ask_the_engine_at_three_qubits():
    from quantpy_amd.geometry import hs_dst, if_dst, trace_dst
    from quantpy_amd.tomography import interval

    assert interval._engine_metric(trace_dst, 6, max_qubits=6) == "trace"
    assert interval._engine_metric(if_dst, 6, max_qubits=6) == "if"
    assert interval._engine_metric(hs_dst, 6, max_qubits=6) is None
    assert interval._engine_metric(lambda a, b: trace_dst(a, b), 6, max_qubits=6) is None  # a custom callable: the host loop
    assert interval._engine_metric(trace_dst, 7, max_qubits=6) is None
    # the call without the keyword answers as it did: a state of six qubits is not the engine's
    assert interval._engine_metric(trace_dst, 6) is None and interval._engine_metric(trace_dst, 5) == "trace"


def test_engine_methods_call_the_entry():
    import inspect

    from quantpy_amd.engine import Engine

    for method in (Engine.metric_dist, Engine.metric_dist_dev):
        assert "lib." + NAME + "(" in inspect.getsource(method) and "64" in method.__doc__
