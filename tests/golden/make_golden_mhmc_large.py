#!/usr/bin/env python3
"""Generate tests/golden/mhmc_large.npz from the *imported reference*: MHMCStateInterval (interval.py:689-750, mhmc.py)
at n = 4 and 5 qubits.

Run with QUANTPY_REF pointing at a checkout of the reference quantpy (the directory holding its `quantpy` package):

    QUANTPY_REF=... PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mhmc_large.py

The reference's interval.py imports cvxopt at module level; cvxopt is not installed, and the chain never calls it, so an
empty placeholder module stands in for it.  The reconstructed state is set directly to the (full-rank) true state: the
reference's numerical-gradient BFGS takes minutes at n = 5, and the chain only needs a positive-definite start.  The
reference's NLL is normalised by the total number of shots, so its target is almost flat: for a Ginibre state nearly
every proposal is accepted.  The true states here are close to the computational basis state |0...0> (0.99 |0><0| +
0.01 Ginibre), whose 'proj-set' frequencies are the most concentrated, and the steps are large enough that some
proposals are rejected in every case (acceptance 0.94-0.98; at n = 5 one in the burn-in and one among the samples).  The n = 5 case also pins
`_proposal_increments`' direct draw at dim 1024 against scipy's frozen multivariate_normal.  Only numbers are written;
the other fixtures and meta.json are not touched.
"""
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["QUANTPY_REF"]


def _import_reference():
    cvx = types.ModuleType("cvxopt")
    cvx.matrix = None
    cvx.solvers = types.SimpleNamespace(options={})
    sys.modules["cvxopt"] = cvx
    sys.path.insert(0, REF)
    import quantpy as qp  # noqa
    import quantpy.mhmc as mhmc  # noqa

    # MHMCStateInterval.setup drops the acceptance rate that MHMC.sample returns: keep the last one
    sample = mhmc.MHMC.sample

    def recording_sample(self, *args, **kwargs):
        samples, rate = sample(self, *args, **kwargs)
        self.last_rate = rate
        return samples, rate

    mhmc.MHMC.sample = recording_sample
    return qp


qp = _import_reference()
warnings.filterwarnings("ignore")


def near_basis_state(rng, d):
    g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = 0.01 * (g @ g.conj().T) / np.trace(g @ g.conj().T)
    rho[0, 0] += 0.99
    return rho


def main():
    cls = np.array([0.1, 0.5, 0.9, 0.99])
    out = {}
    # (n, povm, shots per setting, experiment seed, chain seed, n_points, burn_steps, thinning, step)
    cases = [(4, "proj-set", 1000, 41, 141, 200, 100, 1, 0.3),
             (4, "proj-set", 1000, 42, 142, 100, 60, 2, 1.0),
             (5, "proj-set", 1000, 51, 152, 60, 30, 1, 0.3)]
    for k, (n, povm, shots, seed, chain_seed, n_points, burn, thin, step) in enumerate(cases):
        rho = near_basis_state(np.random.default_rng(seed), 2**n)
        assert np.linalg.eigvalsh(rho).min() > 0
        np.random.seed(seed)
        t = qp.StateTomograph(qp.Qobj(rho))
        t.experiment(shots, povm)
        t.reconstructed_state = qp.Qobj(rho)
        np.random.seed(chain_seed)
        iv = qp.MHMCStateInterval(t, n_points=n_points, step=step, burn_steps=burn, thinning=thin)
        radii = iv(cls)[0]
        key = f"L{k}"
        out[key + "_n"] = np.array(n)
        out[key + "_povm"] = np.array(povm)
        out[key + "_counts"] = np.asarray(t.results, dtype=np.int64)
        out[key + "_state"] = np.asarray(rho, dtype=np.complex128)
        out[key + "_rng_seed"] = np.array(chain_seed)
        out[key + "_args"] = np.array([n_points, burn, thin])
        out[key + "_step"] = np.array(step)
        out[key + "_radii"] = np.asarray(radii, dtype=np.float64)
        out[key + "_all_dist"] = np.asarray(iv.cl_to_dist(np.linspace(0, 1, n_points)), dtype=np.float64)
        out[key + "_final_x"] = np.asarray(iv.chain.x_t, dtype=np.float64)
        out[key + "_rate"] = np.array(iv.chain.last_rate)
        print(f"{key}: n={n} thinning {thin} step {step} acceptance {iv.chain.last_rate:.3f} radii {radii}", flush=True)
    out["n_cases"] = np.array(len(cases))
    out["conf_levels"] = cls
    path = os.path.join(HERE, "mhmc_large.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
