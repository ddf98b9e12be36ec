#!/usr/bin/env python3
"""Generate tests/golden/mle_diet_bits.npz: what the MLE kernels of the library in the tree write for a fixed list of
device-pointer calls, to the bit.  The fixture pins the kernels' results across changes that remove instructions and
keep every floating-point operation and its order (tests/test_gpu_mle_diet_bits.py replays the calls and compares with
np.array_equal).  It was recorded once, on an MI355X, with the library of the commit before the first such change.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mle_diet.py

The script REFUSES to overwrite an existing fixture: recording it again from the code it is there to check would make
the test say nothing.  Whoever changes a floating-point result on purpose deletes the file by hand, with a reason.

The counts are drawn with the CPU oracle (legacy NumPy stream) by the recipes of tests/test_gpu_mle_helper_lift.py and
tests/test_gpu_mle_specialised.py and stored in the fixture, so the test needs the fixture alone.  CASES is shared with
the test: per case the qubit number, POVM, shots per setting, start, iteration cap, whether `fun` is asked for, and the
launch variants ("hw": k_mle_fused_hw, the default at n = 3 from 'lin'; "fused": the one-launch kernel without helpers;
"split": k_mle_start and the eager two-loop pair)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "mle_diet_bits.npz")

# name: (n, povm, shots, init, max_iter, with_fun, variants)
CASES = {
    "n3_ginibre": (3, "proj-set", 100000, "lin", 100, False, ("hw", "fused", "split")),
    "n3_ginibre_fun": (3, "proj-set", 100000, "lin", 100, True, ("hw", "fused", "split")),
    "n3_rank1_lowshot": (3, "proj-set", 1000, "lin", 100, False, ("hw", "fused", "split")),
    "n3_pivot0": (3, "proj-set", 100000, "lin", 100, False, ("hw", "fused", "split")),
    "n3_mixed_start": (3, "proj-set", 100000, "mixed", 30, True, ("fused", "split")),
    "n3_sic": (3, "sic", 100000, "lin", 100, True, ("hw", "fused", "split")),
    "n3_sic_mixed": (3, "sic", 100000, "mixed", 30, True, ("fused", "split")),
    "n1_b5": (1, "proj-set", 400, "lin", 100, True, ("fused", "split")),
    "n1_b17": (1, "proj-set", 400, "lin", 100, True, ("fused", "split")),
    "n1_b17_mixed": (1, "proj-set", 400, "mixed", 100, True, ("fused", "split")),
    "n2_b5": (2, "proj-set", 400, "lin", 100, True, ("fused", "split")),
    "n2_b17": (2, "proj-set", 400, "lin", 100, True, ("fused", "split")),
    "n2_b17_mixed": (2, "proj-set", 400, "mixed", 100, True, ("fused", "split")),
}
DIST_CASE = "n3_ginibre"  # mle_dist_dev runs on this case's counts, against the stored centre


def replay(qp, capi, case, counts, variant, dist_centre=None):
    """One device-pointer call of `case` through `variant` on the process-wide engine -> dict of host arrays
    (complex matrices as float64 pairs).  Sets the options itself and puts the defaults back."""
    import torch

    n, povm, shots, init, max_iter, with_fun, _ = CASES[case]
    eng = qp.get_engine(n)
    a = qp.generate_measurement_matrix(povm, n)
    eng.set_povm(a, np.ones(np.asarray(a).shape[0]) * shots)
    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    nit, nfev, status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda") if with_fun else None
    kw = dict(init=init, max_iter=max_iter, nit=nit, nfev=nfev, fun=fun, status=status)
    out = {}
    try:
        eng.set_option(capi.QT_OPT_MLE_HELPER_WAVE, 1 if variant == "hw" else 0)
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 0 if variant == "split" else 1024)
        if dist_centre is None:
            rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
            eng.mle_dev(cd, rho, **kw)
        else:
            cen = torch.from_numpy(np.ascontiguousarray(dist_centre, dtype=np.complex128)).cuda()
            dist = torch.zeros(b, dtype=torch.float64, device="cuda")
            eng.mle_dist_dev(cd, cen, dist, rho=None, **kw)
        took_hw = eng.mle_helper_wave
        eng.sync()
    finally:
        eng.set_option(capi.QT_OPT_MLE_HELPER_WAVE, 1)
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    assert variant == "hw" or not took_hw, (case, variant)
    out["took_hw"] = np.array(took_hw)  # (a POVM whose tables leave no room for the twins' LDS runs k_mle_fused)
    if dist_centre is None:
        out["rho"] = rho.cpu().numpy().view(np.float64)
    else:
        out["dist"] = dist.cpu().numpy()
    out.update(nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(), status=status.cpu().numpy())
    if with_fun:
        out["fun"] = fun.cpu().numpy()
    return out


def _inputs():
    """case -> counts (B, S, K) int64, drawn with the CPU oracle; and the centre of the distance call."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import quantpy_oracle as qo
    from test_gpu_mle_helper_lift import _classes, _draw, _ginibre

    povm3 = qo.measurement_matrix("proj-set", 3)
    inp = {}
    # the benchmark's stream from trial 10 on: three positive-definite trials and two "go" clipped ones (one negative
    # pivot, the last), in stream order
    stream = _draw(qo, povm3, _ginibre(np.random.default_rng(1234), 8), 100000, 7, 19)[10:]
    cls = _classes(qo, povm3, stream)
    pd_ = [t for t, (e, neg, k, _) in enumerate(cls) if e == 0 and neg == 0][:3]
    go = [t for t, (e, neg, k, _) in enumerate(cls) if e == 1 and neg == 1 and k == 7][:2]
    assert len(pd_) == 3 and len(go) == 2, cls
    inp["n3_ginibre"] = inp["n3_ginibre_fun"] = inp["n3_mixed_start"] = stream[sorted(pd_ + go)]
    # rank 1 at 1e3 shots: several negative eigenvalues (psd_project)
    low = _draw(qo, povm3, _ginibre(np.random.default_rng(77), 8, rank=1), 1000, 8, 5)
    assert all(3 <= e <= 4 for e, _, _, _ in _classes(qo, povm3, low))
    inp["n3_rank1_lowshot"] = low
    # no weight on |0>: the FIRST pivot goes non-positive (wrong pivot order: the serial lift)
    g = _ginibre(np.random.default_rng(5), 8)
    p = np.eye(8)
    p[0, 0] = 0.0
    pgp = p @ g @ p
    piv = _draw(qo, povm3, pgp / np.trace(pgp), 100000, 21, 12)
    cls = _classes(qo, povm3, piv)
    first = [t for t, (e, neg, k, _) in enumerate(cls) if e == 1 and neg == 1 and k == 0][:4]
    other = [t for t in range(len(cls)) if t not in first][:1]
    assert len(first) == 4, cls
    inp["n3_pivot0"] = piv[sorted(first + other)]
    # 'sic': one setting of 64 outcomes, the generic instantiation
    sic3 = qo.measurement_matrix("sic", 3)
    np.random.seed(31)
    bloch = qo.bloch_from_matrix(_ginibre(np.random.default_rng(1234), 8))
    inp["n3_sic"] = inp["n3_sic_mixed"] = np.stack(
        [qo.sample_counts(sic3, bloch, np.ones(sic3.shape[0]) * 100000) for _ in range(5)]).astype(np.int64)
    # n = 1, 2: several trials per wave, partial waves (the recipe of test_gpu_mle_specialised.py)
    for n in (1, 2):
        rng = np.random.default_rng(40 + n)
        povm = qo.measurement_matrix("proj-set", n)
        np.random.seed(50 + n)
        states = [_ginibre(rng, 2**n), _ginibre(rng, 2**n, rank=1)]
        c = np.stack([qo.sample_counts(povm, qo.bloch_from_matrix(states[t % 2]), np.ones(3**n) * 400)
                      for t in range(17)]).astype(np.int64)
        inp[f"n{n}_b5"] = c[:5]
        inp[f"n{n}_b17"] = inp[f"n{n}_b17_mixed"] = c
    assert inp.keys() == CASES.keys()
    return inp, _ginibre(np.random.default_rng(5), 8)


def main():
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: it is recorded once, from the library before the change it checks; not overwritten")
    sys.path.insert(0, ROOT)
    inp, centre = _inputs()
    import quantpy_amd as qp
    from quantpy_amd import _capi

    out = {"dist_centre": centre}
    for case, counts in inp.items():
        out[f"{case}/counts"] = counts
        for variant in CASES[case][6]:
            for k, v in replay(qp, _capi, case, counts, variant).items():
                assert not np.isnan(v).any() and (v != -7).all(), (case, variant, k)
                out[f"{case}/{variant}/{k}"] = v
            print(case, variant, "nit", out[f"{case}/{variant}/nit"], "status", out[f"{case}/{variant}/status"])
    for variant in CASES[DIST_CASE][6]:
        for k, v in replay(qp, _capi, DIST_CASE, inp[DIST_CASE], variant, dist_centre=centre).items():
            assert not np.isnan(v).any(), (variant, k)
            out[f"dist/{variant}/{k}"] = v
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
