#!/usr/bin/env python3
"""Generate tests/golden/polytope5.npz from the *imported reference*: PolytopeStateInterval.setup()
(interval.py:268-335) on a five-qubit tomograph -- 0.9 GHZ + 0.1 mixed state, 'proj-set', 1000 shots per setting,
target the pure GHZ state, n_points = 2: four linear programs with a 7776 x 1023 constraint matrix.

Run ONLY in the development container, where /root/reference exists (about 40 s per program):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_polytope5.py

As make_golden_polytope_fidelity.py (whose `_record` writes the entries): the reference runs behind the recording
cvxopt placeholder of make_golden_polytope.py, whose `solvers.lp` answers with HiGHS.  Only numbers and names are
written: the counts (243 x 32), the widenings, objectives, confidence levels and bounds; of the constraint matrix G
(64 MB) its shape, sum, sum of squares and a few rows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_polytope import _LOG, qp  # noqa: E402  (installs the placeholder and imports the reference)
from make_golden_polytope_fidelity import _record  # noqa: E402

from quantpy.tomography.polytopes.utils import count_delta  # noqa: E402


def main():
    np.random.seed(20261021)
    out = {}
    name, n, n_points = "state5_ghz_projset_1e3", 5, 2
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
    _record(out, name, interval, n_points, freq, tmg.n_measurements, (1,), (0, 1, 3000, 7775))
    out[name + "/deltas"] = np.linspace(count_delta(0, freq, tmg.n_measurements),
                                        count_delta(1 - 1e-7, freq, tmg.n_measurements), n_points)
    out["state_cases"] = np.array([name])
    path = os.path.join(HERE, "polytope5.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
