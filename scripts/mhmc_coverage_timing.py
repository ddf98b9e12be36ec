#!/usr/bin/env python3
"""The chain coverage study (quantpy_amd.metrics.get_CL_list_state_mhmc) on the GHZ state mixed half-and-half with the
identity, 1000 shots per setting ('proj-set'), n = 1, 2, 3, at the study's defaults n_iter = n_points = burn_steps = 1000,
thinning = 1, step = 0.01.  Per n, on the SAME trial counts and estimates:

  fused     ONE qt_mhmc_state_hits over all chains (host-pointer call: counts, estimates, starting points and thresholds
            in, hits and accepted counts out), host clock; and the launch alone on device-resident inputs, HIP events;
  unfused   the composition on entries that predate it, in chunks of CHUNK chains: proposal increments and uniforms drawn
            by NumPy, qt_mhmc_state (the whole chain copied out), qt_chol_unparam of the kept states, qt_hs_dist_dim per
            chain against its own estimate, the hits counted on the host; host clock;
  the two alternate in one process, REPS repeats after WARM warm-ups, min / median / max;
  draws     what drawing costs inside the chain kernel: qt_mhmc_state_hits against qt_mhmc_state reading the same numbers,
            dumped by qt_mhmc_draws, from device memory (and storing the whole chain), on DRAW_CHAINS chains, HIP events; and
            qt_mhmc_draws itself;
  study     get_CL_list_state_mhmc end to end (trial counts, estimates, both qt_chol_param calls, the chains, the levels),
            host clock; and the second of those calls, the test of the eigenvalue floor, alone.

A tree without qt_mhmc_state_hits (the parent of the change that added it) runs the unfused part alone: that is the baseline.
The report goes to standard output and to `--out` (default profiles/mhmc_coverage_timing.txt).
Usage: mhmc_coverage_timing.py [--out PATH] [n_iter [n_points [burn_steps]]]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi, metrics  # noqa: E402
from quantpy_amd.engine import _ptr  # noqa: E402

REPS, WARM = 3, 1
SHOTS, STEP, THINNING = 1000, 0.01, 1
CHUNK = 100         # chains per chunk of the unfused composition (n = 3: 102 MB of increments, as much of chain)
DRAW_CHAINS = 200   # chains of the `draws` comparison (n = 3: 205 MB of increments + 205 MB of chain on the device)
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "mhmc_coverage_timing.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
N_ITER = int(args[0]) if args else 1000
N_POINTS = int(args[1]) if len(args) > 1 else 1000
BURN = int(args[2]) if len(args) > 2 else 1000
TOTAL = BURN + N_POINTS * THINNING
report = open(out_path, "w")


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


def stats(ms):
    ms = np.asarray(ms)
    return f"min {ms.min():10.3f}  median {np.median(ms):10.3f}  max {ms.max():10.3f} ms"


def timed(fn):
    """(host ms, HIP-event ms) of fn(), which leaves the device idle when it returns."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)


def mixed_ghz(n):
    d = 2**n
    psi = np.zeros(d, dtype=np.complex128)
    psi[0] = psi[-1] = 1 / np.sqrt(2)
    return 0.5 * np.outer(psi, psi.conj()) + 0.5 * np.eye(d) / d


FUSED = hasattr(qp.engine.Engine, "mhmc_state_hits")
say(f"mixed GHZ state, {SHOTS} shots per setting, n_iter = {N_ITER}, n_points = {N_POINTS}, burn_steps = {BURN}, thinning = "
    f"{THINNING}, step = {STEP}; {REPS} repeats after {WARM} warm-up; fused entry present: {FUSED}")

for n in (1, 2, 3):
    state = qp.Qobj(mixed_ghz(n))
    tmg = qp.StateTomograph(state, "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=N_ITER, sampler="device", seed=11)
    rho, _ = tmg.point_estimate_batch(counts, method="lin")
    eng = tmg._engine()
    delta = eng.hs_dist(rho, state.matrix)
    x0, status = eng.chol_param(rho)
    assert not status.any()
    dim = eng.D
    res = {}

    def unfused():
        hits = np.zeros(N_ITER, dtype=np.int64)
        acc = np.zeros(N_ITER, dtype=np.int64)
        for lo in range(0, N_ITER, CHUNK):
            hi = min(lo + CHUNK, N_ITER)
            deltas = np.random.standard_normal((hi - lo, TOTAL, dim))
            uniforms = np.random.rand(hi - lo, TOTAL)
            chain, flags = eng.mhmc_state(counts[lo:hi], x0[lo:hi], deltas, uniforms, STEP)
            kept = np.ascontiguousarray(chain[:, BURN::THINNING][:, :N_POINTS])
            mats = eng.chol_unparam(kept.reshape(-1, dim)).reshape(hi - lo, N_POINTS, eng.d, eng.d)
            for c in range(lo, hi):
                hits[c] = (delta[c] > eng.hs_dist(mats[c - lo], rho[c])).sum()
            acc[lo:hi] = flags[:, BURN:].sum(axis=1)
        res["unfused"] = hits, acc

    forms = {"unfused": unfused}
    if FUSED:
        def fused():
            res["fused"] = eng.mhmc_state_hits(counts, rho, x0, delta, 12, BURN, N_POINTS, THINNING, STEP)

        forms["fused  "] = fused
    for fn in forms.values():
        for _ in range(WARM):
            fn()
    times = {name: [] for name in forms}
    for _ in range(REPS):  # alternating, so that whatever else runs on the machine meets both alike
        for name, fn in forms.items():
            times[name].append(timed(fn)[0])
    moved = 2 * N_ITER * TOTAL * dim * 8 / 1e9
    for name in forms:
        say(f"n={n} chains of the study {name}: host {stats(times[name])}"
            + (f"  ({moved:.2f} GB over PCIe)" if name == "unfused" else ""))
    hits_u, acc_u = res["unfused"]
    say(f"n={n} unfused: mean level hits {hits_u.mean():.1f} of {N_POINTS}, acceptance {acc_u.sum() / (N_ITER * N_POINTS * THINNING):.4f}")
    if not FUSED:
        continue
    hits_f, acc_f = res["fused"]
    say(f"n={n} fused  : mean level hits {hits_f.mean():.1f} of {N_POINTS}, acceptance {acc_f.sum() / (N_ITER * N_POINTS * THINNING):.4f}"
        f"  (other random numbers than NumPy's: the same distribution, not the same chains)")
    say(f"n={n} fused faster than unfused by {np.median(times['unfused']) / np.median(times['fused  ']):.1f}x (medians); "
        f"spreads: unfused {np.ptp(times['unfused']):.3f} ms, fused {np.ptp(times['fused  ']):.3f} ms")

    # the launch alone, and what drawing costs in it
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (counts, rho, x0, delta)]

    def launch():
        eng.mhmc_state_hits(*on_dev, 12, BURN, N_POINTS, THINNING, STEP)

    launch()
    say(f"n={n} qt_mhmc_state_hits alone, {N_ITER} chains x {TOTAL} steps: HIP events {stats([timed(launch)[1] for _ in range(REPS)])}")
    nc = min(DRAW_CHAINS, N_ITER)
    part = [t[:nc].contiguous() for t in on_dev]
    d_d = torch.empty((nc, TOTAL, dim), dtype=torch.float64, device=dev)
    u_d = torch.empty((nc, TOTAL), dtype=torch.float64, device=dev)
    chain_d = torch.empty((nc, TOTAL, dim), dtype=torch.float64, device=dev)
    acc_d = torch.zeros((nc, TOTAL), dtype=torch.int32, device=dev)

    def draw():
        eng.mhmc_draws(12, nc, TOTAL, out=(d_d, u_d))

    def reading():  # the chain on numbers read from memory (and the whole chain stored): the kernel that predates the study
        eng._dev_call()
        eng._chk(eng.lib.qt_mhmc_state(eng._h, _ptr(part[0]), nc, _ptr(part[2]), _ptr(d_d), _ptr(u_d), TOTAL, STEP, _ptr(chain_d),
                                       _ptr(acc_d), _capi.QT_DEVICE_PTR))

    def drawing():
        res["part"] = eng.mhmc_state_hits(*part, 12, BURN, N_POINTS, THINNING, STEP)

    for fn in (draw, reading, drawing):
        fn()
    t_draw = [timed(draw)[1] for _ in range(REPS)]
    t = {"reading": [], "drawing": []}
    for _ in range(REPS):
        t["reading"].append(timed(reading)[1])
        t["drawing"].append(timed(drawing)[1])
    same = int((acc_d[:, BURN:].sum(dim=1) == res["part"][1]).sum())
    say(f"n={n} draws, {nc} chains x {TOTAL} steps: qt_mhmc_draws {stats(t_draw)}")
    say(f"n={n} draws: qt_mhmc_state reading them   {stats(t['reading'])}")
    say(f"n={n} draws: qt_mhmc_state_hits drawing   {stats(t['drawing'])}   (accepted counts equal on {same} of {nc} chains)")
    say(f"n={n} draws: per step of a chain {1e6 * np.median(t['reading']) / TOTAL:.0f} ns reading, "
        f"{1e6 * np.median(t['drawing']) / TOTAL:.0f} ns drawing (Philox, log, sin / cos, and the distance of a kept step)")
    del d_d, u_d, chain_d, acc_d

    def study():
        study.levels = metrics.get_CL_list_state_mhmc(state, n_iter=N_ITER, n_points=N_POINTS, n_measurements=SHOTS, step=STEP,
                                                      burn_steps=BURN, thinning=THINNING, seed=11)

    def floor_test():  # the study's second qt_chol_param: a Cholesky factor of estimate - _PD_FLOOR * 1
        eng.chol_param(rho - metrics._PD_FLOOR * np.eye(eng.d))

    floor_test()
    say(f"n={n} study: its floor test alone (qt_chol_param of {N_ITER} shifted estimates): host {stats([timed(floor_test)[0] for _ in range(REPS)])}")
    study()
    host = [timed(study)[0] for _ in range(REPS)]
    lv = study.levels
    say(f"n={n} study end to end: host {stats(host)} | levels: mean {lv.mean():.3f}, share below 0.9: {(lv < 0.9).mean():.3f}")
report.close()
