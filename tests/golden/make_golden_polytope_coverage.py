#!/usr/bin/env python3
"""Generate tests/golden/polytope_coverage.npz from the *imported reference* (quantpy/tomography/polytopes: utils.py,
verification.py) and from its recorded results (polytopes/results/*.pkl).

Run ONLY in the development container, where /root/reference exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_polytope_coverage.py

cvxopt is not installed and nothing here solves a program, so the reference is imported behind an inert cvxopt
placeholder.  Only numbers are written; the other fixtures are not touched.

1. formula/<group>/...: count tables, widenings, the reference's float64 count_confidence and the same formula in
   np.longdouble (64-bit mantissa on x86) on the same clipped float64 frequencies.  A group is one shape and one
   shot count.  Asserted: every group has >= 5 widenings whose confidence lies in (1e-6, 1 - 1e-9).
2. study/<name>/...: seeded runs of the reference's own test_qst / test_qpt; the reference's count_delta and its
   np.min(b - polytope_prod) are wrapped to record every (trial, level) delta, hit and membership margin.  Asserted:
   the smallest |min(b - t) + 1e-15| of a stored study is >= 1e-8 (the seed is advanced until it is).
3. published/...: the recorded 10 000-trial tables of the reference's Verification notebook.
"""
import os
import pickle
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
EPS = 1e-15
LEVELS = np.array([0, 0.1, 0.5, 0.9, 0.99, 0.999, 1 - 1e-7])


def _import_reference():
    cvx = types.ModuleType("cvxopt")
    cvx.matrix = lambda *a, **k: None
    cvx.solvers = types.SimpleNamespace(options={})
    sys.modules["cvxopt"] = cvx
    sys.path.insert(0, REF)
    import quantpy as qp  # noqa
    from quantpy.tomography.polytopes import utils, verification

    return qp, utils, verification


qp, utils, verification = _import_reference()
warnings.filterwarnings("ignore")


def ginibre(rng, d, rank):
    g = rng.standard_normal((d, rank)) + 1j * rng.standard_normal((d, rank))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


# ---- 1. formula cases ---------------------------------------------------------------------------------------------
def confidence_extended(delta, frequencies, n_measurements):
    """utils.count_confidence with every operation in np.longdouble (the inputs are the float64 values)."""
    ld = np.longdouble
    f = np.asarray(frequencies, dtype=np.float64).astype(ld)
    n = np.asarray(n_measurements, dtype=np.float64).astype(ld)
    eps = ld(np.float64(EPS))
    top = ld(np.float64(1 - EPS))
    s = np.clip(f + ld(np.float64(delta)), eps, top)
    kl = f * np.log(f / s) + (1 - f) * np.log((1 - f) / (1 - s))
    kl = np.where(s < top, kl, ld(np.inf))
    e = np.exp(-n[:, None] * kl)
    e = np.where(np.abs(f - 1) < 2 * eps, ld(0), e)
    return np.prod(np.maximum(1 - np.sum(e, axis=-1), ld(0)))


def formula_group(rng, shape, shots, unequal):
    """Two tables of one shape: multinomial draws of random distributions, then a setting with its whole mass on one
    outcome (f = 1, zero counts beside it) and a few more zeroed entries."""
    *lead, S, K = shape
    R = int(np.prod(lead, dtype=np.int64)) * S
    n_set = np.full(S, shots, dtype=np.int64)
    if unequal:
        n_set = np.maximum((shots * rng.uniform(0.5, 1.5, S)).astype(np.int64), 2)
    tables, widenings, ref, ext = [], [], [], []
    for _ in range(2):
        p = rng.dirichlet(np.full(K, 0.7), size=R)
        n_rows = np.tile(n_set, R // S)
        c = np.array([rng.multinomial(n_rows[r], p[r]) for r in range(R)], dtype=np.int64)
        r1 = rng.integers(R)
        c[r1] = 0
        c[r1, rng.integers(K)] = n_rows[r1]
        for _ in range(3):  # moved, not dropped: the row sums stay the shots
            r, a, b = rng.integers(R), rng.integers(K), rng.integers(K)
            if a != b:
                c[r, b] += c[r, a]
                c[r, a] = 0
        freq = np.clip(c.reshape(*lead, S, K) / n_set[:, None], EPS, 1 - EPS)
        base = np.concatenate(([1e-10, 1e-7, 1e-5, 0.5, 0.9, 1 - 1e-12, 1.0], np.geomspace(1e-4, 0.3, 25)))
        near = np.array([utils.count_delta(cl, freq, n_set) for cl in (1e-4, 0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.999)])
        d = np.concatenate((base, near))
        tables.append(c)
        widenings.append(d)
        ref.append([utils.count_confidence(x, freq, n_set) for x in d])
        ext.append([confidence_extended(x, freq.reshape(R, K), np.tile(n_set, R // S)) for x in d])
    ref = np.array(ref, dtype=np.float64)
    ext_ld = np.array(ext, dtype=np.longdouble)
    informative = (ext_ld > 1e-6) & (ext_ld < 1 - 1e-9)
    assert informative.sum(axis=1).min() >= 5, (shape, shots, informative.sum(axis=1))
    e_ref = float(np.max(np.abs(ref.astype(np.longdouble) - ext_ld)))
    # the extended value as a float64 pair (hi + lo), so that the fixture does not depend on the longdouble format
    hi = ext_ld.astype(np.float64)
    lo = (ext_ld - hi.astype(np.longdouble)).astype(np.float64)
    return {"counts": np.array(tables), "shots": np.tile(n_set, R // S).astype(np.float64), "deltas": np.array(widenings),
            "ref": ref, "ext_hi": hi, "ext_lo": lo, "e_ref": np.array(e_ref), "R": np.array(R), "K": np.array(K)}


# ---- 2. seeded studies ----------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for `np` and `count_delta` inside the reference's verification module."""

    def __init__(self):
        self.deltas, self.margins, self.freqs, self.shots = [], [], [], None

    def count_delta(self, cl, frequencies, n_measurements):
        if cl == LEVELS[0]:
            self.freqs.append(np.array(frequencies))
            self.shots = np.array(n_measurements)
        d = utils.count_delta(cl, frequencies, n_measurements)
        self.deltas.append(d)
        return d

    def __getattr__(self, name):
        return getattr(np, name)

    def min(self, a, *args, **kwargs):
        m = np.min(a, *args, **kwargs)
        self.margins.append(m)
        return m


def run_study(kind, obj, shots, trials, seed, **kwargs):
    while True:
        rec = _Recorder()
        verification.np = rec
        verification.count_delta = rec.count_delta
        verification.tqdm = lambda it: it
        try:
            np.random.seed(seed)
            fn = verification.test_qst if kind == "state" else verification.test_qpt
            fractions = fn(obj, LEVELS, shots, trials, **kwargs)
            after = np.random.random()
        finally:
            verification.np = np
            verification.count_delta = utils.count_delta
        margins = np.array(rec.margins).reshape(trials, len(LEVELS))
        smallest = np.min(np.abs(margins + EPS))
        if smallest >= 1e-8:
            break
        seed += 1
    freqs = np.array(rec.freqs)  # (T, S, K) or (T, D, S, K)
    counts = np.rint(freqs * rec.shots[:, None]).astype(np.int64)
    assert np.array_equal(np.clip(counts / rec.shots[:, None], EPS, 1 - EPS), freqs)
    hits = margins > -EPS
    assert np.array_equal(hits.mean(axis=0), fractions)
    return {"seed": np.array(seed), "shots": np.array(shots), "trials": np.array(trials), "counts": counts,
            "deltas": np.array(rec.deltas).reshape(trials, len(LEVELS)), "hits": hits.astype(np.uint8),
            "fractions": np.asarray(fractions), "min_margin": np.array(smallest), "random_after": np.array(after)}


def main():
    rng = np.random.default_rng(20261016)
    out = {"levels": LEVELS}

    groups = [("s1_1e2", (3, 2), 100, False), ("s1_1e1", (3, 2), 10, False), ("s1_1e7", (3, 2), 10**7, False),
              ("s2_1e3", (9, 4), 1000, False), ("s2_uneq", (9, 4), 5000, True), ("s3_1e4", (27, 8), 10**4, False),
              ("s4_1e3", (81, 16), 1000, True), ("s5_1e4", (243, 32), 10**4, False), ("p3_1e4", (64, 27, 8), 10**4, False),
              ("p1_1e5", (4, 3, 2), 10**5, False)]
    for name, shape, shots, unequal in groups:
        g = formula_group(rng, shape, shots, unequal)
        for k, v in g.items():
            out[f"formula/{name}/{k}"] = v
        print("formula", name, shape, shots, "e_ref %.2e" % g["e_ref"])
    out["formula_groups"] = np.array([g[0] for g in groups])

    studies = [
        # name, kind, n, rank (0: channel), shots, trials, keyword arguments
        ("qst1_pure_1e2", "state", 1, 1, 100, 300, {}),
        ("qst1_mixed_1e5", "state", 1, 2, 10**5, 300, {}),
        ("qst2_pure_1e3", "state", 2, 1, 1000, 200, {}),
        ("qst2_mixed_1e4", "state", 2, 3, 10**4, 200, {}),
        ("qst3_pure_1e3", "state", 3, 1, 1000, 100, {}),
        ("qst3_mixed_1e2", "state", 3, 8, 100, 100, {}),
        ("qpt1_sic_1e3", "channel", 1, 0, 1000, 200, {"input_states": "sic"}),
        ("qpt1_proj4_1e2", "channel", 1, 0, 100, 200, {"input_states": "proj4"}),
        ("qpt2_sic_1e4", "channel", 2, 0, 10**4, 48, {"input_states": "sic"}),
        ("qpt2_proj4_1e3", "channel", 2, 0, 1000, 48, {"input_states": "proj4"}),
    ]
    for i, (name, kind, n, rank, shots, trials, kw) in enumerate(studies):
        if kind == "state":
            rho = ginibre(rng, 2**n, rank)
            obj = qp.Qobj(rho)
            out[f"study/{name}/rho"] = rho
        else:
            p = 0.1 + 0.05 * (i % 3)
            obj = qp.channel.depolarizing(p=p, n_qubits=n)
            out[f"study/{name}/depolarizing_p"] = np.array(p)
            out[f"study/{name}/input_states"] = np.array(kw["input_states"])
        out[f"study/{name}/n_qubits"] = np.array(n)
        s = run_study(kind, obj, shots, trials, 7000 + 10 * i, **kw)
        for k, v in s.items():
            out[f"study/{name}/{k}"] = v
        print("study", name, "seed", int(s["seed"]), "fractions", s["fractions"], "min margin %.2e" % s["min_margin"])
    out["studies"] = np.array([s[0] for s in studies])

    res = os.path.join(REF, "polytopes", "results")
    rows, labels = [], []
    with open(os.path.join(res, "states_qubits_10k.pkl"), "rb") as fh:
        obj = pickle.load(fh)
    cl = np.asarray(obj["cl"], dtype=np.float64)
    for n, row in enumerate(obj["results"], start=1):
        rows.append(row)
        labels.append((0, n, 10**4))  # (0 = GHZ state / 1 = depolarizing(0.1) channel with "sic" inputs, qubits, shots)
    with open(os.path.join(res, "processes_qubits_10k.pkl"), "rb") as fh:
        obj = pickle.load(fh)
    assert np.array_equal(cl, obj["cl"])
    for n, row in enumerate(obj["results"], start=1):
        rows.append(row)
        labels.append((1, n, 10**4))
    with open(os.path.join(res, "processes_meas.pkl"), "rb") as fh:
        obj = pickle.load(fh)
    assert np.array_equal(cl, obj["cl"])
    for k, row in enumerate(obj["results"]):
        rows.append(row)
        labels.append((1, 1, 10 ** (2 + k)))
    out["published/levels"] = cl
    out["published/fractions"] = np.asarray(rows, dtype=np.float64)
    out["published/rows"] = np.asarray(labels, dtype=np.int64)
    out["published/trials"] = np.array(10000)
    assert out["published/fractions"].shape == (12, 18)

    path = os.path.join(HERE, "polytope_coverage.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
