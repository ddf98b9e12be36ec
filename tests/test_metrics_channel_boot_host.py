"""Host: quantpy_amd.metrics.get_CL_list_channel_boot refuses bad arguments before anything touches the GPU, the refusal
of get_CL_list_channel(interval='boot') names it, and the C entries behind it are declared in the public header."""
import inspect
import os
import re

import pytest

from quantpy_amd import _capi, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_argument_errors():
    with pytest.raises(ValueError, match="sampler"):
        metrics.get_CL_list_channel_boot(None, sampler="cupy")
    for kw in (dict(n_iter=0), dict(n_points=0), dict(n_iter=-3), dict(n_points=-1)):
        with pytest.raises(ValueError, match="positive"):
            metrics.get_CL_list_channel_boot(None, **kw)


def test_signature_follows_the_reference():
    params = list(inspect.signature(metrics.get_CL_list_channel_boot).parameters.values())
    names = [p.name for p in params]
    assert names == ["channel", "n_iter", "n_points", "n_measurements", "method", "povm", "input_states", "cptp",
                     "states_init", "states_est_method", "sampler", "seed", "chunk", "return_details"]
    defaults = {p.name: p.default for p in params[1:]}
    assert defaults == dict(n_iter=1000, n_points=1000, n_measurements=1000, method="lifp", povm="proj-set",
                            input_states="proj4", cptp=True, states_init="lin", states_est_method="lin", sampler="device",
                            seed=None, chunk=None, return_details=False)
    assert all(p.kind is p.KEYWORD_ONLY for p in params[-4:])


def test_the_old_refusal_names_the_study():
    with pytest.raises(NotImplementedError, match="boot") as err:
        metrics.get_CL_list_channel(None, interval="boot")
    assert "get_CL_list_channel_boot" in str(err.value)
    assert "get_CL_list_channel_boot" in metrics.get_CL_list_channel.__doc__


@pytest.mark.parametrize("name", ["qt_lifp_dist_group_batch", "qt_process_born_probs"])
def test_entries_are_declared(name):
    with open(os.path.join(ROOT, "include", "qtomo.h")) as fh:
        header = fh.read()
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
    assert m, name
    assert name in _capi.SIGNATURES and len(_capi.SIGNATURES[name][1]) == m.group(1).count(",") + 1
