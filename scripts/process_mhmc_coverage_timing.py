#!/usr/bin/env python3
"""The process chain coverage study (quantpy_amd.metrics.get_CL_list_channel_mhmc) on the depolarizing channel (p = 0.1),
1000 shots per setting ('proj-set', 'proj4' input states), n = 1, 2, at the study's defaults n_iter = n_points =
burn_steps = 1000, thinning = 1, step = 0.01.  Per n, on the SAME trial counts and estimates:

  fused     ONE qt_mhmc_process_hits over all chains (host-pointer call: counts, estimates and thresholds in, hits and
            accepted counts out), host clock; and the launch alone on device-resident inputs, HIP events;
  unfused   the composition on entries that predate it, in chunks of CHUNK[n] chains: proposal increments and uniforms
            drawn by NumPy, qt_mhmc_process (the whole chain copied out), the real parts of the kept states through
            qt_hs_dist_dim per chain against its own estimate, the hits counted on the host; host clock;
  the two alternate in one process, REPS repeats after a warm-up (the fused call in full, the unfused composition on one
  chunk), min / median / max;
  study     get_CL_list_channel_mhmc end to end (trial counts, estimates, the chains, the levels), host clock.

A tree without qt_mhmc_process_hits (the parent of the change that added it) runs the unfused part alone: that is the
baseline.  The report goes to standard output and to `--out` (default profiles/process_mhmc_coverage_timing.txt).
Usage: process_mhmc_coverage_timing.py [--out PATH] [--n 1,2] [n_iter [n_points [burn_steps]]]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import metrics  # noqa: E402

REPS = 3
SHOTS, STEP, THINNING, NOISE = 1000, 0.01, 1, 0.1
CHUNK = {1: 250, 2: 50}  # chains per chunk of the unfused composition (n = 2: 205 MB of increments, 410 MB of chain)
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "process_mhmc_coverage_timing.txt")
sizes = (1, 2)
while args[:1] and args[0].startswith("--"):
    if args[0] == "--out":
        out_path = args[1]
    elif args[0] == "--n":
        sizes = tuple(int(v) for v in args[1].split(","))
    args = args[2:]
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


FUSED = hasattr(qp.engine.Engine, "mhmc_process_hits")
say(f"depolarizing channel (p = {NOISE}), {SHOTS} shots per setting, n_iter = {N_ITER}, n_points = {N_POINTS}, burn_steps = "
    f"{BURN}, thinning = {THINNING}, step = {STEP}; {REPS} repeats after a warm-up; fused entry present: {FUSED}")

for n in sizes:
    channel = qp.channel.depolarizing(NOISE, n)
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=N_ITER, sampler="device", seed=11)
    choi = tmg.point_estimate_batch(counts, method="lifp")
    eng = tmg._engine()
    delta = eng.hs_dist(choi, channel.choi.matrix)
    ne = eng.D * eng.D
    chunk = min(CHUNK[n], N_ITER)
    res = {}

    def unfused(stop=N_ITER):
        hits = np.zeros(N_ITER, dtype=np.int64)
        acc = np.zeros(N_ITER, dtype=np.int64)
        for lo in range(0, stop, chunk):
            hi = min(lo + chunk, N_ITER)
            deltas = np.random.standard_normal((hi - lo, TOTAL, ne))
            uniforms = np.random.rand(hi - lo, TOTAL)
            chain, flags = eng.mhmc_process(counts[lo:hi], choi[lo:hi], deltas, uniforms, STEP)
            kept = np.ascontiguousarray(chain[:, BURN::THINNING][:, :N_POINTS].real)
            for c in range(lo, hi):
                hits[c] = (delta[c] > eng.hs_dist(kept[c - lo], choi[c])).sum()
            acc[lo:hi] = flags[:, BURN:].sum(axis=1)
        res["unfused"] = hits, acc

    forms = {"unfused": unfused}
    unfused(chunk)  # warm-up: one chunk
    if FUSED:
        def fused():
            res["fused"] = eng.mhmc_process_hits(counts, choi, choi, delta, 12, BURN, N_POINTS, THINNING, STEP)

        forms["fused  "] = fused
        fused()
    times = {name: [] for name in forms}
    for _ in range(REPS):  # alternating, so that whatever else runs on the machine meets both alike
        for name, fn in forms.items():
            times[name].append(timed(fn)[0])
            say(f"n={n}   {name}: {times[name][-1]:10.3f} ms")
    moved = N_ITER * TOTAL * ne * (8 + 16) / 1e9
    for name in forms:
        say(f"n={n} chains of the study {name}: host {stats(times[name])}"
            + (f"  (chunks of {chunk} chains; {moved:.2f} GB over PCIe)" if name == "unfused" else ""))
    hits_u, acc_u = res["unfused"]
    say(f"n={n} unfused: mean level hits {hits_u.mean():.1f} of {N_POINTS}, acceptance {acc_u.sum() / (N_ITER * N_POINTS * THINNING):.4f}")
    if not FUSED:
        continue
    hits_f, acc_f = res["fused"]
    say(f"n={n} fused  : mean level hits {hits_f.mean():.1f} of {N_POINTS}, acceptance {acc_f.sum() / (N_ITER * N_POINTS * THINNING):.4f}"
        f"  (other random numbers than NumPy's: the same distribution, not the same chains)")
    say(f"n={n} fused faster than unfused by {np.median(times['unfused']) / np.median(times['fused  ']):.1f}x (medians); "
        f"spreads: unfused {np.ptp(times['unfused']):.3f} ms, fused {np.ptp(times['fused  ']):.3f} ms")

    # the launch alone
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (counts, choi, choi, delta)]

    def launch():
        eng.mhmc_process_hits(*on_dev, 12, BURN, N_POINTS, THINNING, STEP)

    launch()
    ev = [timed(launch)[1] for _ in range(REPS)]
    say(f"n={n} qt_mhmc_process_hits alone, {N_ITER} chains x {TOTAL} steps: HIP events {stats(ev)}"
        f"  ({1e3 * np.median(ev) / TOTAL:.2f} us per step of the launch)")

    def study():
        study.levels = metrics.get_CL_list_channel_mhmc(channel, n_iter=N_ITER, n_points=N_POINTS, n_measurements=SHOTS,
                                                        step=STEP, burn_steps=BURN, thinning=THINNING, seed=11)

    study()
    host = [timed(study)[0] for _ in range(REPS)]
    lv = study.levels
    say(f"n={n} study end to end: host {stats(host)} | levels: mean {lv.mean():.3f}, share below 0.9: {(lv < 0.9).mean():.3f}")
report.close()
