"""The host helpers of the polytope interval (reference polytopes/utils.py:4-27) against the deltas and confidence levels
the reference computed for tests/golden/polytope.npz.  No GPU."""
import numpy as np
import pytest
from conftest import load_golden

from quantpy_amd.tomography.interval import count_confidence, count_delta


def _frequencies(g, name):
    counts = g[name + "/counts"]
    shots = counts.sum(-1).astype(np.float64)
    return np.clip(counts / shots[:, None], 1e-15, 1 - 1e-15), shots


@pytest.mark.parametrize("name", list(load_golden("polytope")["polytope_cases"]))
def test_count_delta_and_confidence_match_reference(name):
    g = load_golden("polytope")
    f, shots = _frequencies(g, name)
    deltas = np.linspace(count_delta(0, f, shots), count_delta(1 - 1e-7, f, shots), int(g[name + "/n_points"]))
    assert np.array_equal(deltas[[0, -1]], g[name + "/delta_range"])
    conf = np.array([count_confidence(d, f, shots) for d in deltas])
    ref = g[name + "/conf_levels"]
    assert np.all(np.abs(conf - ref) <= 1e-15 * np.abs(ref))


def test_count_confidence_edge_cases():
    f = np.array([[1 - 1e-15, 1e-15], [0.5, 0.5]])
    shots = np.array([10.0, 10.0])
    assert count_confidence(0.0, f, shots) == 0.0
    assert 0.0 < count_confidence(0.3, f, shots) < 1.0
