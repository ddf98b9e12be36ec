"""Host: the surface of the trace distance / infidelity of dim x dim matrices (qt_metric_dist_dim) without a GPU -- the C
entry is declared and exported, the binding has its ten arguments, the rules a caller relies on stand where the entry is
declared, and the intervals ask the engine for these distances up to five qubits."""
import ctypes
import os
import re

from quantpy_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qt_metric_dist_dim"


def test_entry_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/qtomo.h"
    assert NAME in _capi.SIGNATURES and len(_capi.SIGNATURES[NAME][1]) == m.group(1).count(",") + 1 == 10
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    # declared under the entry for n <= 3, whose argument order it follows with `dim` behind `metric`
    assert header.index("int qt_metric_dist_group_batch(") < m.start()
    assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == \
        ["h", "metric", "dim", "rho", "B", "centres", "G", "g0", "dist", "flags"]


def test_header_comment_states_the_rules():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    at = header.index("int " + NAME + "(")
    doc = header[header.rindex("/*", 0, at):at]
    for word in ("geometry.py:23-38", ":41-56", "HERMITIAN", "1e-15", "NaN", "QT_ERR_UNSUPPORTED", "QT_ERR_ARG",
                 "2, 4, 8, 16, 32"):
        assert word in doc, word


def test_intervals_ask_the_engine_up_to_five_qubits():
    from quantpy_amd.geometry import hs_dst, if_dst, trace_dst
    from quantpy_amd.tomography import interval

    for n in range(1, 6):
        assert interval._engine_metric(trace_dst, n) == "trace"
        assert interval._engine_metric(if_dst, n) == "if"
        assert interval._engine_metric(hs_dst, n) is None
        assert interval._engine_metric(lambda a, b: trace_dst(a, b), n) is None  # a custom callable: the host loop
    assert interval._engine_metric(trace_dst, 6) is None  # a three-qubit Choi matrix (dim 64)


def test_engine_has_both_forms():
    from quantpy_amd.engine import Engine

    assert callable(Engine.metric_dist_dim) and callable(Engine.metric_dist_dim_dev)
