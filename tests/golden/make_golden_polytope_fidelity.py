#!/usr/bin/env python3
"""Generate tests/golden/polytope_fidelity.npz from the *imported reference*: PolytopeProcessInterval.setup()
(interval.py:338-418) at n = 1 and n = 2, and PolytopeStateInterval.setup() (interval.py:268-335) at n = 4.

Run ONLY in the development container, where /root/reference exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_polytope_fidelity.py

The reference runs behind the recording cvxopt placeholder of make_golden_polytope.py (imported from there), whose
`solvers.lp` saves its arguments and answers with HiGHS; agreement with cvxopt itself is not verified.  Only numbers
and names are written.  The dense constraint matrix G (1.1 MB at n = 2, 2.6 MB for the four-qubit state) and the
four-qubit POVM tensor do not go in: the POVM and the input states are stored by name, and of G its shape, sum, sum of
squares and a few rows; the right-hand sides h at a few widenings.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_polytope import _LOG, qp  # noqa: E402  (installs the placeholder and imports the reference)

from quantpy.tomography.polytopes.utils import count_confidence, count_delta  # noqa: E402


def _record(out, name, interval, n_points, freq, shots, h_rows, g_rows):
    lps = [e for e in _LOG if e[0] == "lp"]
    assert len(lps) == 2 * n_points
    G = lps[0][2]
    assert all(np.array_equal(e[2], G) for e in lps)
    assert all(np.array_equal(lps[2 * r][1], -lps[2 * r + 1][1]) for r in range(n_points))
    deltas = np.linspace(count_delta(0, freq, shots), count_delta(1 - 1e-7, freq, shots), n_points)
    conf = np.array([count_confidence(d, freq, shots) for d in deltas])
    assert np.array_equal(conf, interval.cl_to_dist_min.x)
    g_rows = np.arange(G.shape[0]) if g_rows is None else np.asarray(g_rows)
    out[name + "/n_points"] = np.array(n_points)
    out[name + "/delta_range"] = np.array([deltas[0], deltas[-1]])
    out[name + "/conf_levels"] = conf
    out[name + "/G_shape"] = np.array(G.shape)
    out[name + "/G_sum"] = np.array(G.sum())
    out[name + "/G_sumsq"] = np.array((G * G).sum())
    out[name + "/G_rows"] = g_rows
    out[name + "/G_sample"] = G[g_rows]
    out[name + "/c"] = lps[0][1]
    out[name + "/h_rows"] = np.asarray(h_rows)
    out[name + "/h"] = np.array([lps[2 * r][3] for r in h_rows])
    out[name + "/lp_obj"] = np.array([[lps[2 * r][5], lps[2 * r + 1][5]] for r in range(n_points)])
    out[name + "/lp_status"] = np.array([[lps[2 * r][4], lps[2 * r + 1][4]] for r in range(n_points)], dtype=np.int8)
    out[name + "/dist_min"] = np.asarray(interval.cl_to_dist_min.y, dtype=np.float64)
    out[name + "/dist_max"] = np.asarray(interval.cl_to_dist_max.y, dtype=np.float64)
    print(name, G.shape, "lp statuses", np.unique(out[name + "/lp_status"]))


def main():
    np.random.seed(20261017)
    out = {}
    # processes: depolarizing(0.1) measured with 'sic' inputs and 'proj-set', 1000 shots; target: the identity channel
    pnames = []
    for name, n, n_points, h_rows, g_rows in (("proc1_sic_projset_1e3", 1, 200, range(0, 200, 20), None),
                                              ("proc2_sic_projset_1e3", 2, 12, (0, 5, 11), (0, 1, 100, 287, 288, 430, 575))):
        channel, target = qp.channel.depolarizing(0.1, n), qp.channel.depolarizing(0, n)
        tmg = qp.ProcessTomograph(channel, input_states="sic")
        tmg.experiment(1000, "proj-set")
        _LOG.clear()
        interval = qp.PolytopeProcessInterval(tmg, n_points=n_points, target_channel=target)
        interval.setup()
        shots = tmg.tomographs[0].n_measurements
        freq = np.asarray([np.clip(t.results / t.n_measurements[:, None], 1e-15, 1 - 1e-15) for t in tmg.tomographs])
        out[name + "/counts"] = np.asarray([t.results for t in tmg.tomographs], dtype=np.int64)
        out[name + "/shots"] = np.asarray(shots, dtype=np.float64)
        out[name + "/n_qubits"] = np.array(n)
        out[name + "/povm"] = np.array("proj-set")
        out[name + "/input_states"] = np.array("sic")
        out[name + "/states_matrix"] = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements], dtype=np.float64)
        out[name + "/depolarizing"] = np.array([0.1, 0.0])  # the measured channel, the target
        out[name + "/true_bloch"] = np.asarray(channel.choi.bloch, dtype=np.float64)
        out[name + "/target_bloch"] = np.asarray(target.choi.bloch, dtype=np.float64)
        _record(out, name, interval, n_points, freq, shots, h_rows, g_rows)
        pnames.append(name)
    # state: a depolarised four-qubit GHZ state, 'proj-set', 1000 shots; target: GHZ
    name, n, n_points = "state4_ghz_projset_1e3", 4, 8
    target = qp.qobj.GHZ(n)
    state = qp.channel.depolarizing(0.1, n).transform(target)
    tmg = qp.StateTomograph(state)
    tmg.experiment(1000, "proj-set")
    _LOG.clear()
    interval = qp.PolytopeStateInterval(tmg, n_points=n_points, target_state=target)
    interval.setup()
    freq = np.clip(tmg.results / tmg.n_measurements[:, None], 1e-15, 1 - 1e-15)
    out[name + "/counts"] = np.asarray(tmg.results, dtype=np.int64)
    out[name + "/shots"] = np.asarray(tmg.n_measurements, dtype=np.float64)
    out[name + "/n_qubits"] = np.array(n)
    out[name + "/povm"] = np.array("proj-set")
    out[name + "/true_bloch"] = np.asarray(state.bloch, dtype=np.float64)
    out[name + "/target_bloch"] = np.asarray(target.bloch, dtype=np.float64)
    _record(out, name, interval, n_points, freq, tmg.n_measurements, (0, 7), (0, 1, 500, 647, 648, 1295))
    out["process_cases"] = np.array(pnames)
    out["state_cases"] = np.array([name])
    path = os.path.join(HERE, "polytope_fidelity.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
