#!/usr/bin/env python3
"""Generate tests/golden/polytope.npz from the *imported reference* (PolytopeStateInterval, interval.py:268-335, and
MomentFidelityStateInterval, interval.py:113-160).

Run ONLY in the development container, where /root/reference exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_polytope.py

cvxopt is not installed, so the reference is imported behind a RECORDING cvxopt placeholder: its `solvers.lp(c, G, h)`
and `solvers.socp(c, Gq, hq, A, b)` save their arguments and answer with an independent exact solver -- HiGHS
(scipy.optimize.linprog) for the LPs, SLSQP polished by Newton on the KKT system for the SOCPs -- returning None where cvxopt would (infeasible /
unbounded), so the reference's own loop turns the answers into dist_min / dist_max exactly as it would with cvxopt.
The deltas and confidence levels come from the reference's pure-NumPy polytopes/utils.py.  Only numbers are written;
the other fixtures and meta.json are not touched.
"""
import os
import sys
import types
import warnings

import numpy as np
from scipy.optimize import linprog, minimize, root

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

_LOG = []


def _matrix(data, size=None, tc=None):
    a = np.array(data, dtype=np.float64)
    if a.ndim == 1:
        a = a[:, None]
    if size is not None:
        a = a.reshape(size, order="F")  # cvxopt is column-major
    return a


def _lp(c, G, h, *args, **kwargs):
    c, G, h = (np.asarray(v, dtype=np.float64) for v in (c, G, h))
    res = linprog(c.ravel(), A_ub=G, b_ub=h.ravel(), bounds=[(None, None)] * G.shape[1], method="highs")
    obj = res.fun if res.status == 0 else None
    _LOG.append(("lp", c.ravel().copy(), G.copy(), h.ravel().copy(), res.status, np.nan if obj is None else obj))
    return {"primal objective": obj, "status": "optimal" if obj is not None else "infeasible"}


def _socp(c, Gq, hq, A, b, *args, **kwargs):
    c = np.asarray(c, dtype=np.float64).ravel()
    G, h = np.asarray(Gq[0], dtype=np.float64), np.asarray(hq[0], dtype=np.float64).ravel()
    A, b = np.asarray(A, dtype=np.float64), np.asarray(b, dtype=np.float64).ravel()
    # ||h[1:] - G[1:] x|| <= h[0] - G[0] x,  A x = b   (here G[0] = 0, G[1:] = I)
    centre, radius = h[1:], h[0]
    x0 = centre.copy()
    x0[0] = b[0]
    cons = [{"type": "eq", "fun": lambda x: A @ x - b},
            {"type": "ineq", "fun": lambda x: radius**2 - np.sum((centre - G[1:] @ x) ** 2)}]
    res = minimize(lambda x: c @ x, x0, jac=lambda x: c, constraints=cons, method="SLSQP",
                   options={"ftol": 1e-15, "maxiter": 1000})
    feasible = radius**2 >= (centre[0] - b[0]) ** 2
    obj = None
    if feasible:
        # polish SLSQP's point with Newton on the KKT system (c + lam (x - centre) + nu A^T = 0, A x = b, on the sphere)
        x = res.x
        dx = x - centre
        lam = -(c[1:] @ dx[1:]) / (dx[1:] @ dx[1:])
        nu = -(c[0] + lam * dx[0])

        def kkt(v):
            x, lam, nu = v[:-2], v[-2], v[-1]
            return np.concatenate([c + lam * (x - centre) + nu * A[0], A @ x - b, [np.sum((x - centre) ** 2) - radius**2]])

        sol = root(kkt, np.concatenate([x, [lam, nu]]), method="hybr", options={"xtol": 1e-15})
        obj = float(c @ sol.x[:-2])
        assert abs(obj - res.fun) < 1e-7 and np.abs(kkt(sol.x)).max() < 1e-12
    _LOG.append(("socp", c.copy(), radius, centre.copy(), b.copy(), np.nan if obj is None else obj))
    return {"primal objective": obj}


def _import_reference():
    cvx = types.ModuleType("cvxopt")
    cvx.matrix = _matrix
    cvx.solvers = types.SimpleNamespace(options={}, lp=_lp, socp=_socp)
    sys.modules["cvxopt"] = cvx
    sys.path.insert(0, REF)
    import quantpy as qp  # noqa

    return qp


qp = _import_reference()
warnings.filterwarnings("ignore")


def ginibre(rng, d, rank):
    g = rng.standard_normal((d, rank)) + 1j * rng.standard_normal((d, rank))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def main():
    rng = np.random.default_rng(20261016)
    np.random.seed(20261016)
    out = {}
    # (name, n, povm, shots, rank of the true state (1 = pure), n_points, warm-start second run)
    cases = [
        ("p1_projset_pure_1e2", 1, "proj-set", 100, 1, 1000, None),
        ("p1_projset_mixed_1e5", 1, "proj-set", 100000, 2, 1000, None),
        ("p2_projset_mixed_1e3", 2, "proj-set", 1000, 4, 1000, None),
        ("p2_proj_pure_1e3", 2, "proj", 1000, 1, 1000, None),
        ("p2_sic_mixed_1e5", 2, "sic", 100000, 3, 1000, None),
        ("p2_projset_warm", 2, "proj-set", 100, 2, 1000, ("proj-set", 1000)),
        ("p3_projset_mixed_1e3", 3, "proj-set", 1000, 8, 300, None),
    ]
    names = []
    for name, n, povm, shots, rank, n_points, warm in cases:
        d = 2**n
        tmg = qp.StateTomograph(qp.Qobj(ginibre(rng, d, rank)))
        tmg.experiment(shots, povm)
        if warm is not None:
            tmg.experiment(warm[1], warm[0], warm_start=True)
        _LOG.clear()
        interval = qp.PolytopeStateInterval(tmg, n_points=n_points)
        interval.setup()
        lps = [e for e in _LOG if e[0] == "lp"]
        assert len(lps) == 2 * n_points
        G = lps[0][2]
        assert all(np.array_equal(e[2], G) for e in lps)
        from quantpy.tomography.polytopes.utils import count_confidence, count_delta

        freq = np.clip(tmg.results / tmg.n_measurements[:, None], 1e-15, 1 - 1e-15)
        deltas = np.linspace(count_delta(0, freq, tmg.n_measurements), count_delta(1 - 1e-7, freq, tmg.n_measurements),
                             n_points)
        assert np.array_equal(np.linspace(deltas[0], deltas[-1], n_points), deltas)
        conf = np.array([count_confidence(dl, freq, tmg.n_measurements) for dl in deltas])
        assert np.array_equal(conf, interval.cl_to_dist_min.x)
        out[name + "/counts"] = np.asarray(tmg.results, dtype=np.int64)
        out[name + "/povm"] = np.asarray(tmg.povm_matrix, dtype=np.float64)
        out[name + "/target"] = np.asarray(tmg.state.bloch, dtype=np.float64)
        out[name + "/n_points"] = np.array(n_points)
        out[name + "/delta_range"] = np.array([deltas[0], deltas[-1]])  # the deltas are np.linspace over this range
        out[name + "/conf_levels"] = conf
        out[name + "/G"] = G
        out[name + "/c"] = lps[0][1]
        # To keep the fixture small, the LP results are stored at 101 evenly spaced deltas (first and last included)
        # and the right-hand sides h = clip(f + delta) - W[:, 0] at 11 of them; statuses and confidence levels at all.
        rows = np.unique(np.linspace(0, n_points - 1, 101).round().astype(np.int64))
        h_rows = rows[::10]
        out[name + "/lp_rows"] = rows
        out[name + "/h_rows"] = h_rows
        out[name + "/h"] = np.array([lps[2 * r][3] for r in h_rows])
        out[name + "/lp_obj"] = np.array([[lps[2 * r][5], lps[2 * r + 1][5]] for r in rows])
        out[name + "/lp_status"] = np.array([[e[4] for e in lps[0::2]], [e[4] for e in lps[1::2]]], dtype=np.int8).T
        out[name + "/dist_min"] = np.asarray(interval.cl_to_dist_min.y, dtype=np.float64)[rows]
        out[name + "/dist_max"] = np.asarray(interval.cl_to_dist_max.y, dtype=np.float64)[rows]
        names.append(name)
        print(name, G.shape, "lp statuses", np.unique(out[name + "/lp_status"]))
    # the moment-fidelity interval: two targets per case (the true state and the default, the reconstructed state)
    mcases = [("m1_projset_1e3", 1, "proj-set", 1000, 2, True), ("m2_projset_1e3", 2, "proj-set", 1000, 4, True),
              ("m2_projset_default", 2, "proj-set", 1000, 1, False)]
    mnames = []
    for name, n, povm, shots, rank, with_target in mcases:
        d = 2**n
        tmg = qp.StateTomograph(qp.Qobj(ginibre(rng, d, rank)))
        tmg.experiment(shots, povm)
        _LOG.clear()
        interval = qp.MomentFidelityStateInterval(tmg, target_state=tmg.state if with_target else None)
        interval.setup()
        soc = [e for e in _LOG if e[0] == "socp"]
        levels = interval.cl_to_dist_min.x
        assert len(soc) == 2 * len(levels)
        out[name + "/counts"] = np.asarray(tmg.results, dtype=np.int64)
        out[name + "/povm"] = np.asarray(tmg.povm_matrix, dtype=np.float64)
        out[name + "/target"] = np.asarray(interval.target_state.bloch, dtype=np.float64)
        out[name + "/with_target"] = np.array(with_target)
        out[name + "/levels"] = np.asarray(levels)
        out[name + "/cl_to_dist"] = np.asarray(interval.cl_to_dist(levels), dtype=np.float64)
        out[name + "/socp_c"] = soc[0][1]
        out[name + "/socp_radius"] = np.array([e[2] for e in soc[0::2]])
        out[name + "/socp_centre"] = soc[0][3]
        out[name + "/socp_obj"] = np.array([[e[5] for e in soc[0::2]], [e[5] for e in soc[1::2]]]).T
        out[name + "/dist_min"] = np.asarray(interval.cl_to_dist_min.y, dtype=np.float64)
        out[name + "/dist_max"] = np.asarray(interval.cl_to_dist_max.y, dtype=np.float64)
        mnames.append(name)
        print(name, "socp", len(soc))
    out["polytope_cases"] = np.array(names)
    out["moment_cases"] = np.array(mnames)
    np.savez_compressed(os.path.join(HERE, "polytope.npz"), **out)
    print("wrote", os.path.join(HERE, "polytope.npz"))


if __name__ == "__main__":
    main()
