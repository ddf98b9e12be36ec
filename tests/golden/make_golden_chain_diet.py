#!/usr/bin/env python3
"""Generate tests/golden/chain_diet_bits.npz: what the n = 3 entries that use the 64-lane reductions of qt_wave.h (and
are not replayed by mle_diet_bits.npz) write for a fixed list of calls, to the bit.  It was recorded once, on an MI355X,
with the library of the commit before the second "instruction diet" (cross-row reduction stages without row masks, trace
reductions that start where two diagonal lanes meet, the Gauss-Jordan inverse unrolled in natural pivot order, the
squaring loop's control): such a change keeps every floating-point operation that reaches a result, and its order, so
what a call writes stays equal under np.array_equal (tests/test_gpu_chain_diet_bits.py replays the calls).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chain_diet.py

The script REFUSES to overwrite an existing fixture (see make_golden_mle_diet.py).

Five trials, B = 5 = one full workgroup of four trials plus a partial one, all 'proj-set' at 1e5 shots per setting, one per
class of the unprojected linear-inversion matrix:
  0  positive definite;
  1  one negative pivot, the last (the natural-order lift: four squarings on the benchmark's stream);
  2  one negative pivot that is not the last (the run-time pivot order);
  3  two negative pivots (the eigensolver);
  4  all counts zero: every frequency is 0 / 0, so every entry derived from the counts is NaN.
The matrix-valued entries (qt_chol_param, qt_hs_dist_dim, qt_metric_dist_group_batch) get the unprojected
linear-inversion matrices of the five trials, as the library wrote them; the chains of qt_mhmc_state start from the
Cholesky parameters of the clipped ones.  The MLE calls run on classes 0 - 2 (MLE_PICK): one launch at B = 5, the split
pair at B = 1030."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "chain_diet_bits.npz")
SHOTS = 100000
NAN_TRIAL = 4
MLE_PICK = (0, 1, 2, 1, 0)  # classes 0 - 2, five trials
SPLIT_B = 1030
MHMC_STEPS = 3
MHMC_STEP = 0.01


def _f(a):
    """complex arrays as float64 pairs: np.array_equal on the bits' values, NaN handled by the caller"""
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


def _set_povm(qp):
    eng = qp.get_engine(3)
    a = qp.generate_measurement_matrix("proj-set", 3)
    eng.set_povm(a, np.ones(np.asarray(a).shape[0]) * SHOTS)
    return eng


def replay_entries(qp, capi, counts, deltas, uniforms):
    """The five entries on the five trials -> dict of host arrays."""
    eng = _set_povm(qp)
    b, d, dd = counts.shape[0], eng.d, eng.D
    out = {}
    # qt_lin_batch, unprojected and with the physical clip (raw calls: no exception on a status)
    for physical in (0, 1):
        rho = np.full((b, d, d), -7.0, dtype=np.complex128)
        bloch = np.full((b, dd), -7.0)
        st = np.full(b, -7, dtype=np.int32)
        eng._chk(eng.lib.qt_lin_batch(eng._h, counts.ctypes.data, b, physical, rho.ctypes.data, bloch.ctypes.data,
                                      st.ctypes.data, capi.QT_HOST_PTR))
        tag = "lin_phys" if physical else "lin_raw"
        out[f"{tag}/rho"], out[f"{tag}/bloch"], out[f"{tag}/status"] = _f(rho), bloch, st
        if physical:
            clipped = rho.copy()
        else:
            raw = rho.copy()
    x, st = eng.chol_param(raw)
    out["chol_raw/x"], out["chol_raw/status"] = x, st
    x0, st = eng.chol_param(clipped)
    out["chol_phys/x"], out["chol_phys/status"] = x0, st
    out["hs/dist"] = eng.hs_dist(raw, clipped[0])
    for metric in ("trace", "if"):
        out[f"metric_{metric}/one"] = eng.metric_dist(raw, clipped[0], metric)
        out[f"metric_{metric}/table"] = eng.metric_dist(clipped, clipped[:3], metric, g0=1)
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, MHMC_STEP)
    out["mhmc/chain"], out["mhmc/accepted"] = chain, acc
    return out


def replay_mle(qp, capi, counts, split):
    """One device-pointer MLE call from 'lin': the one-launch kernel, or k_mle_start and the two-loop pair."""
    import torch

    eng = _set_povm(qp)
    b, d = counts.shape[0], eng.d
    cd = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int64)).cuda()
    nit, nfev, status = (torch.full((b,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    fun = torch.zeros(b, dtype=torch.float64, device="cuda")
    rho = torch.zeros((b, d, d), dtype=torch.complex128, device="cuda")
    try:
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 0 if split else 1024)
        eng.mle_dev(cd, rho, init="lin", max_iter=100, nit=nit, nfev=nfev, fun=fun, status=status)
        took_hw = eng.mle_helper_wave
        eng.sync()
    finally:
        eng.set_option(capi.QT_OPT_MLE_FUSED_MAX_WAVES, 1024)
    assert took_hw == (not split), (split, took_hw)
    return dict(rho=rho.cpu().numpy().view(np.float64), nit=nit.cpu().numpy(), nfev=nfev.cpu().numpy(),
                status=status.cpu().numpy(), fun=fun.cpu().numpy())


def mle_counts(counts, split):
    c = counts[list(MLE_PICK)]
    return np.ascontiguousarray(np.resize(c, (SPLIT_B,) + c.shape[1:])) if split else c


def _inputs():
    """The five trials' counts (5, S, K) int64, drawn with the CPU oracle, and the chains' random numbers."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import quantpy_oracle as qo
    from test_gpu_mle_helper_lift import _classes, _draw, _ginibre

    povm = qo.measurement_matrix("proj-set", 3)
    stream = _draw(qo, povm, _ginibre(np.random.default_rng(1234), 8), SHOTS, 7, 19)[10:]
    cls = _classes(qo, povm, stream)
    pd_ = next(t for t, (e, neg, k, _) in enumerate(cls) if e == 0 and neg == 0)
    go = next(t for t, (e, neg, k, _) in enumerate(cls) if e == 1 and neg == 1 and k == 7)
    g = _ginibre(np.random.default_rng(5), 8)
    p = np.eye(8)
    p[0, 0] = 0.0
    pgp = p @ g @ p
    piv = _draw(qo, povm, pgp / np.trace(pgp), SHOTS, 21, 12)
    first = next(t for t, (e, neg, k, _) in enumerate(_classes(qo, povm, piv)) if e == 1 and neg == 1 and k == 0)
    r6 = _draw(qo, povm, _ginibre(np.random.default_rng(106), 8, rank=6), SHOTS, 32, 40)
    two = next(t for t, (e, neg, k, _) in enumerate(_classes(qo, povm, r6)) if e == 2 and neg == 2)
    counts = np.stack([stream[pd_], stream[go], piv[first], r6[two], np.zeros_like(stream[0])]).astype(np.int64)
    rng = np.random.default_rng(2024)
    deltas = rng.standard_normal((5, MHMC_STEPS, 64))
    uniforms = rng.random((5, MHMC_STEPS))
    return counts, deltas, uniforms


def main():
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: it is recorded once, from the library before the change it checks; not overwritten")
    sys.path.insert(0, ROOT)
    counts, deltas, uniforms = _inputs()
    import quantpy_amd as qp
    from quantpy_amd import _capi

    out = {"counts": counts, "deltas": deltas, "uniforms": uniforms}
    for k, v in replay_entries(qp, _capi, counts, deltas, uniforms).items():
        out[f"entries/{k}"] = v
        print(k, "NaN rows:", sorted(set(np.argwhere(np.isnan(v))[:, 0].tolist())) if v.dtype.kind == "f" else v)
    for split in (False, True):
        tag = "mle_split" if split else "mle_hw"
        for k, v in replay_mle(qp, _capi, mle_counts(counts, split), split).items():
            assert not np.isnan(v).any() and (v != -7).all(), (tag, k)
            out[f"{tag}/{k}"] = v[:5] if split else v
            if split:  # the batch repeats five trials: so do the results (only five rows are stored)
                assert np.array_equal(v, np.resize(v[:5], v.shape)), (tag, k)
        print(tag, "nit", out[f"{tag}/nit"], "status", out[f"{tag}/status"])
    np.savez_compressed(FIXTURE, **out)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


if __name__ == "__main__":
    main()
