#!/usr/bin/env python3
"""The chain coverage study of a three-qubit channel (quantpy_amd.metrics.get_CL_list_channel_mhmc_large) on the
depolarizing channel (p = 0.1), 10 000 shots per setting ('proj-set', 'proj4' input states), step = 1e-5, thinning = 1.

  study     get_CL_list_channel_mhmc_large end to end (trial counts, estimates, the chains, the levels), host clock, in 'hs'
            and 'trace', for n_iter = 64 and n_iter = 1000 at n_points = burn_steps = 1000 (`--large-points P`: the
            n_iter = 1000 run with n_points = burn_steps = P instead, said in the report);
  chains    the chains alone on device-resident inputs (qt_mhmc_process_large_hits / _metric_hits), HIP events, and from
            them the time per step;
  unfused   at n_iter = 64, once: the composition of entries this study does not use, in pieces of PIECE steps --
            qt_mhmc_draws_dim (the numbers written out), qt_mhmc_process from the last state of the piece before (the whole
            piece of the chain copied out), the real parts of the kept states through hs_dist / metric_dist per chain --
            host clock, with the bytes it moves;
  kernels   `--kernel-stats CSV`: the per-kernel share of a step, from the kernel_stats.csv of one
            `rocprofv3 --kernel-trace --stats -- python process_mhmc_large_coverage_timing.py --steps-only` run (1000
            chains, 10 burn-in steps and 20 kept ones, 'trace': nothing else is launched in that mode).

The report goes to standard output and to `--out` (default profiles/process_mhmc_large_coverage_timing.txt).
Usage: process_mhmc_large_coverage_timing.py [--out PATH] [--large-points P] [--kernel-stats CSV] [--no-unfused] [--steps-only]"""
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import metrics  # noqa: E402

SHOTS, STEP, THINNING, NOISE, N = 10000, 1e-5, 1, 0.1, 3
POINTS = 1000  # n_points = burn_steps of the study
PIECE = 100    # steps per piece of the unfused composition at 64 chains: 210 MB of increments, 419 MB of chain
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "process_mhmc_large_coverage_timing.txt")
large_points, stats_csv, with_unfused, steps_only = POINTS, None, True, False
while args:
    if args[0] == "--out":
        out_path, args = args[1], args[2:]
    elif args[0] == "--large-points":
        large_points, args = int(args[1]), args[2:]
    elif args[0] == "--kernel-stats":
        stats_csv, args = args[1], args[2:]
    elif args[0] == "--no-unfused":
        with_unfused, args = False, args[1:]
    elif args[0] == "--steps-only":
        steps_only, args = True, args[1:]
    else:
        raise SystemExit(__doc__)

channel = qp.channel.depolarizing(NOISE, N)


def trials(n_iter):
    """(engine, counts, estimates) of n_iter tomographies, as the study forms them"""
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=n_iter, sampler="device", seed=11)
    choi = tmg.point_estimate_batch(counts, method="lifp")
    return tmg._engine(), counts, choi


if steps_only:  # for the profiler: the chains of 1000 trials, 30 steps, and nothing else behind the set-up
    eng, counts, choi = trials(1000)
    delta = eng.distance(choi, channel.choi.matrix, "trace")
    hits, acc = eng.mhmc_process_hits(counts, choi, choi, delta, 12, 10, 20, 1, STEP, metric="trace")
    print("steps-only: accepted", int(acc.sum()), "of", 20 * 1000)
    sys.exit(0)

report = open(out_path, "w")


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


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


say(f"three-qubit depolarizing channel (p = {NOISE}), {SHOTS} shots per setting, step = {STEP}, thinning = {THINNING}; every "
    f"figure is one run after a warm-up of 3 chains x 12 steps (a study takes seconds: the spread of the n_iter = 64 runs is "
    f"shown by their two repeats)")
eng, counts, choi = trials(3)
for metric in (None, "trace"):
    eng.mhmc_process_hits(counts, choi, choi, eng.distance(choi, channel.choi.matrix, metric), 12, 2, 5, 2, STEP, metric=metric)

for n_iter, points, reps in ((64, POINTS, 2), (1000, large_points, 1)):
    total = points + points * THINNING
    note = "" if points == POINTS else f"  (n_points = burn_steps = {points}, NOT the defaults' {POINTS}: the run is long)"
    for dst in ("hs", "trace"):
        for rep in range(reps):
            def study():
                study.out = metrics.get_CL_list_channel_mhmc_large(channel, n_iter=n_iter, n_points=points,
                                                                   n_measurements=SHOTS, step=STEP, burn_steps=points,
                                                                   thinning=THINNING, seed=11, dst=dst, return_details=True)

            host = timed(study)[0]
            out = study.out
            lv = out["levels"]
            say(f"study  n_iter={n_iter:5d} n_points=burn_steps={points:5d} dst={dst:5s}: host {host:10.1f} ms end to end | "
                f"acceptance {out['acceptance_rate'].mean():.3f}, mean level {lv.mean():.3f}, share below 0.9: "
                f"{(lv < 0.9).mean():.3f}{note}")
    eng, counts, choi = trials(n_iter)
    dev = torch.device("cuda", eng.device)
    for dst in ("hs", "trace"):
        metric = None if dst == "hs" else dst
        delta = eng.distance(choi, channel.choi.matrix, metric)
        on_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (counts, choi, choi, delta)]

        def launch():
            eng.mhmc_process_hits(*on_dev, 12, points, points, THINNING, STEP, metric=metric)

        ev = timed(launch)[1]
        say(f"chains n_iter={n_iter:5d} n_points=burn_steps={points:5d} dst={dst:5s}: HIP events {ev:10.1f} ms for {total} steps "
            f"({ev / total:.3f} ms per step){note}")

if with_unfused:
    n_iter, points = 64, POINTS
    eng, counts, choi = trials(n_iter)
    for dst in ("hs", "trace"):
        metric = None if dst == "hs" else dst
        delta = eng.distance(choi, channel.choi.matrix, metric)

        def unfused():
            hits = np.zeros(n_iter, dtype=np.int64)
            acc = np.zeros(n_iter, dtype=np.int64)
            x = choi
            for first in range(0, 2 * points, PIECE):
                deltas, uniforms = eng.mhmc_draws_dim(4096, 12, n_iter, PIECE, first_step=first)
                chain, flags = eng.mhmc_process(counts, x, deltas, uniforms, STEP)
                x = np.ascontiguousarray(chain[:, -1])
                if first >= points:
                    kept = np.ascontiguousarray(chain.real)
                    for c in range(n_iter):
                        hits[c] += (delta[c] > eng.distance(kept[c], choi[c], metric)).sum()
                    acc += flags.sum(axis=1)
            unfused.out = hits, acc

        host = timed(unfused)[0]
        f_hits, f_acc = eng.mhmc_process_hits(counts, choi, choi, delta, 12, points, points, THINNING, STEP, metric=metric)
        u_hits, u_acc = unfused.out
        moved = n_iter * 2 * points * 4096 * (8 + 8 + 16) / 1e9 + n_iter * points * 4096 * 16 / 1e9
        say(f"unfused n_iter={n_iter} n_points=burn_steps={points} dst={dst:5s}: host {host:10.1f} ms in pieces of {PIECE} steps "
            f"({moved:.1f} GB between host and device) | accepted equal to the fused entry's: {np.array_equal(u_acc, f_acc)}, "
            f"hits equal: {np.array_equal(u_hits, f_hits)}")

if stats_csv:
    with open(stats_csv) as fh:
        rows = list(csv.DictReader(fh))
    name_key = next(k for k in rows[0] if k.lower().startswith("name"))
    total_key = next(k for k in rows[0] if "total" in k.lower())
    calls_key = next(k for k in rows[0] if k.lower().startswith("calls"))
    chain_kernels = ("k_mhmc64", "k_cptp_project64", "k_fwd64_nll", "k_metric_dist_dim64", "k_psd_sqrt_dim64")
    rows = [r for r in rows if any(k in r[name_key] for k in chain_kernels)]
    whole = sum(float(r[total_key]) for r in rows)
    say("kernels of the chains, rocprofv3 --kernel-trace --stats, 1000 chains x 30 steps (10 burn-in, 20 kept), dst='trace':")
    for r in sorted(rows, key=lambda r: -float(r[total_key])):
        t, calls = float(r[total_key]), int(r[calls_key])
        say(f"  {r[name_key].split('(')[0][:60]:60s} calls {calls:4d}  mean {t / calls / 1e3:9.1f} us  share {100 * t / whole:5.1f} %")
report.close()
