"""No GPU: the two chain entries in trace distance and infidelity -- qt_mhmc_state_metric_hits,
qt_mhmc_process_metric_hits -- as the header declares them, the library exports them and _capi binds them, and the `dst`
argument of the three coverage studies that grew one."""
import ctypes
import inspect
import os
import re

import pytest

from quantpy_amd import _capi, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"qt_mhmc_state_metric_hits": "qt_mhmc_state_hits", "qt_mhmc_process_metric_hits": "qt_mhmc_process_hits"}


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        return fh.read()


def _declaration(header, name):
    """(start of the declaration, its argument names)"""
    m = re.search(r"^int " + name + r"\((.*?)\);", header, re.S | re.M)
    assert m, name
    return m.start(), [a.split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]


def _comment_before(header, at):
    end = header.rindex("*/", 0, at)
    return header[header.rindex("/*", 0, end):end]


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_entries_are_declared_exported_and_bound(header, name):
    at, names = _declaration(header, name)
    sib_at, sib_names = _declaration(header, PAIRS[name])
    assert sib_at < at  # under its *_hits sibling
    nxt = re.compile(r"^int qt_\w+\(", re.M).search(header, sib_at + 1)
    assert nxt.start() == at  # ... directly
    assert len(names) == 17 and names[1] == "metric"
    assert names[:1] + names[2:] == sib_names and len(sib_names) == 16  # the sibling's arguments, `metric` behind the handle
    assert hasattr(ctypes.CDLL(_capi.LIB_PATH), name)
    restype, argtypes = _capi.SIGNATURES[name]
    sib_restype, sib_argtypes = _capi.SIGNATURES[PAIRS[name]]
    assert restype is sib_restype and len(argtypes) == 17
    assert argtypes[1] is ctypes.c_int and argtypes[:1] + argtypes[2:] == sib_argtypes


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_header_comments_state_the_rules(header, name):
    text = " ".join(_comment_before(header, _declaration(header, name)[0]).replace("*", " ").split())
    for rule in ("geometry.py:23-38", ":41-56", "HERMITIAN", "1e-15", "NaN", "QT_ERR_ARG", "QT_ERR_UNSUPPORTED",
                 "QT_METRIC_TRACE", "QT_METRIC_INFIDELITY", "bit-identical", "without a launch"):
        assert rule in text, (name, rule)


def test_dst_is_keyword_only_on_the_studies():
    for fn in (metrics.get_CL_list_state_mhmc, metrics.get_CL_list_channel_mhmc):
        p = inspect.signature(fn).parameters["dst"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "hs"
    p = inspect.signature(metrics.get_CL_list_channel_boot_dst).parameters["dst"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == "hs"
    # ... on a study of its own: the argument list of get_CL_list_channel_boot is the one its callers know
    assert "dst" not in inspect.signature(metrics.get_CL_list_channel_boot).parameters


STUDIES = [metrics.get_CL_list_state_mhmc, metrics.get_CL_list_channel_mhmc, metrics.get_CL_list_channel_boot_dst]


@pytest.mark.parametrize("fn", STUDIES, ids=lambda f: f.__name__)
def test_unknown_distance_is_refused_before_any_gpu_use(fn, monkeypatch):
    """`_distance_name`'s ValueError, with neither a tomograph nor an engine built (the state / channel is never looked
    at); the older argument errors still come first."""
    from quantpy_amd.tomography.process import ProcessTomograph
    from quantpy_amd.tomography.state import StateTomograph

    def no_tomograph(*a, **k):
        raise AssertionError("the refusal must come before the tomograph is built")

    for cls in (StateTomograph, ProcessTomograph):
        monkeypatch.setattr(cls, "__init__", no_tomograph)
        monkeypatch.setattr(cls, "_engine", no_tomograph)
    with pytest.raises(ValueError, match="`dst`"):
        fn(None, dst="fro")
    with pytest.raises(ValueError, match="`dst`"):
        fn(None, dst=abs)
    with pytest.raises(ValueError, match="positive"):
        fn(None, n_iter=0, dst="fro")
    with pytest.raises(ValueError, match="sampler"):
        fn(None, sampler="sobol", dst="fro")
    if fn is not metrics.get_CL_list_channel_boot_dst:
        with pytest.raises(ValueError, match="thinning"):
            fn(None, thinning=0, dst="fro")
        with pytest.raises(ValueError, match="burn_steps"):
            fn(None, burn_steps=-1, dst="fro")


@pytest.mark.parametrize("dst", ["hs", "trace", "if"])
def test_three_qubit_channel_is_still_refused_before_the_tomograph_is_built(dst, monkeypatch):
    import quantpy_amd as qp
    from quantpy_amd.tomography.process import ProcessTomograph

    def no_tomograph(*a, **k):
        raise AssertionError("the refusal must come before the tomograph is built")

    monkeypatch.setattr(ProcessTomograph, "__init__", no_tomograph)
    monkeypatch.setattr(ProcessTomograph, "_engine", no_tomograph)
    with pytest.raises(NotImplementedError, match="one and two qubits"):
        metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.1, 3), n_iter=2, n_points=3, burn_steps=1, dst=dst)


def test_engine_refuses_an_unknown_metric_name_before_the_library_is_called():
    from quantpy_amd.engine import Engine

    class Probe:
        _METRICS = Engine._METRICS
        _metric_code = Engine._metric_code

    for method in (Engine.mhmc_state_hits, Engine.mhmc_process_hits):
        assert inspect.signature(method).parameters["metric"].default is None
        with pytest.raises(ValueError, match="metric must be"):
            method(Probe(), None, None, None, None, 1, 0, 1, 1, 0.1, metric="hs")
