"""Host: the surface of the batched trace distance / infidelity without a GPU -- the C entry is declared and exported, the
binding carries its constants, and the argument errors of metrics.get_CL_list_state_boot come before any GPU use."""
import ctypes
import os
import re

import numpy as np
import pytest

from quantpy_amd import _capi, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "qt_metric_dist_group_batch"


def test_entry_is_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + NAME + r"\(([^;]*)\);", header)
    assert m, "not declared in include/qtomo.h"
    assert NAME in _capi.SIGNATURES and len(_capi.SIGNATURES[NAME][1]) == m.group(1).count(",") + 1 == 9
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), NAME)
    # the rules a caller relies on are stated where the entry is declared
    doc = header[header.rindex("/*", 0, m.start()):m.start()]
    for word in ("geometry.py:23-38", ":41-56", "HERMITIAN", "1e-15", "NaN", "QT_ERR_UNSUPPORTED", "QT_ERR_ARG"):
        assert word in doc, word


def test_constants():
    assert (_capi.QT_METRIC_TRACE, _capi.QT_METRIC_INFIDELITY) == (0, 1)
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        assert re.search(r"QT_METRIC_TRACE = 0,\s*QT_METRIC_INFIDELITY = 1", fh.read())


def test_batch_functions_are_exported():
    import quantpy_amd as qp
    from quantpy_amd import geometry

    assert qp.trace_dst_batch is geometry.trace_dst_batch and qp.if_dst_batch is geometry.if_dst_batch
    with pytest.raises(ValueError, match="expected"):
        qp.trace_dst_batch(np.eye(2), np.eye(2))  # one matrix is not a batch


def test_study_argument_errors_before_any_gpu_use():
    fn = metrics.get_CL_list_state_boot  # (the state is never looked at: these come in front of everything else)
    for dst in ("hs", "trace", "if"):
        with pytest.raises(ValueError, match="positive"):
            fn(None, dst=dst, n_iter=0)
        with pytest.raises(ValueError, match="positive"):
            fn(None, dst=dst, n_points=0)
        with pytest.raises(ValueError, match="sampler"):
            fn(None, dst=dst, sampler="sobol")
        with pytest.raises(NotImplementedError, match="method_boot"):
            fn(None, dst=dst, method_boot="mle-constr")
    with pytest.raises(ValueError, match="dst"):
        fn(None, dst="bures")
    with pytest.raises(ValueError, match="dst"):
        fn(None, dst=lambda a, b: 0.0)


@pytest.mark.parametrize("dst", ["trace", "if"])
@pytest.mark.parametrize("interval", ["gamma", "boot"])
def test_the_general_study_still_refuses_and_names_the_new_one(interval, dst):
    with pytest.raises(NotImplementedError, match="Hilbert-Schmidt.*get_CL_list_state_boot"):
        metrics.get_CL_list_state(None, interval=interval, dst=dst)
    with pytest.raises(NotImplementedError, match="Hilbert-Schmidt") as err:
        metrics.get_CL_list_channel(None, dst=dst)
    assert "get_CL_list_state_boot" not in str(err.value)  # (the channel studies have no such form)
