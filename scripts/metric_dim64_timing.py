#!/usr/bin/env python3
"""Trace distance and infidelity of 64 x 64 matrices on the engine (qt_metric_dist_mat) and the two intervals of a
three-qubit channel built on them.

  kernel    `Engine.metric_dist_dev` on random full-rank density matrices resident on the device, 4096 of them at
            d = 64 and, for context, 16 384 at d = 32, both metrics, against one centre (G = 1) and against a table of
            G = 1000 centres; HIP events on the engine's stream, REPS repeats after WARM warm-ups, median (min - max),
            and the ratio of the time per matrix at d = 64 to that at d = 32 (the rotation count predicts 8).  The
            infidelity includes its set-up launch (the roots of the G centres).
  interval  `BootstrapProcessInterval(n_points=1000, method='lifp', sampler='device').setup()` and
            `MHMCProcessInterval(n_points=1000, burn_steps=1000).setup()` on a three-qubit depolarizing channel with
            dst='trace', end to end on the host clock, IREPS repeats after one warm-up, median (min - max).

A tree whose engine refuses d = 64 (the parent of the change that added it) runs `interval` alone: there the distances are
one scipy.linalg.sqrtm per sample on the host, and that is the baseline.  The report goes to standard output and is
APPENDED to `--out` (default profiles/metric_dim64_timing.txt), so that runs of the two trees can alternate into one file.
Usage: metric_dim64_timing.py [--out PATH] [--label TEXT] [kernel] [interval]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi  # noqa: E402

BATCH, TABLE = {32: 16384, 64: 4096}, 1000
REPS, WARM = 20, 3
IREPS, N_POINTS, BURN, SHOTS = 3, 1000, 1000, 1000
args = sys.argv[1:]
out_path, label = os.path.join(ROOT, "profiles", "metric_dim64_timing.txt"), "this tree"
while args[:1] and args[0] in ("--out", "--label"):
    if args[0] == "--out":
        out_path = args[1]
    else:
        label = args[1]
    args = args[2:]
parts = args or ["kernel", "interval"]
report = open(out_path, "a")
HAVE = "qt_metric_dist_mat" in _capi.SIGNATURES


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


def stats(ms):
    ms = np.asarray(ms)
    return f"median {np.median(ms):10.4f}  ({ms.min():10.4f} - {ms.max():10.4f}) ms"


def full_rank(g, count, d):
    m = g.standard_normal((count, d, d)) + 1j * g.standard_normal((count, d, d))
    rho = m @ m.conj().transpose(0, 2, 1)
    return rho / np.trace(rho, axis1=1, axis2=2).real[:, None, None]


say(f"[{label}] distances of 64 x 64 matrices on the engine: {HAVE}")
if "kernel" in parts and HAVE:
    say(f"kernel: metric_dist_dev, matrices on the device, HIP events, {REPS} repeats after {WARM} warm-ups")
    eng = qp.get_engine(3)
    per_matrix = {}
    for d in (32, 64):
        g = np.random.default_rng(d)
        b = BATCH[d]
        rho = torch.from_numpy(full_rank(g, b, d)).cuda()
        table = torch.from_numpy(full_rank(g, TABLE, d)).cuda()
        dist = torch.empty(b, dtype=torch.float64, device="cuda")
        for metric in ("trace", "if"):
            for centres in (table[0], table):
                ms = []
                for rep in range(WARM + REPS):
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    eng.metric_dist_dev(rho, centres, dist, metric)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= WARM:
                        ms.append(e0.elapsed_time(e1))
                groups = centres.shape[0] if centres.dim() == 3 else 1
                per_matrix[d, metric, groups] = 1e6 * np.median(ms) / b
                say(f"  d={d} B={b} {metric:5s} G={groups:4d}: {stats(ms)}   ({per_matrix[d, metric, groups]:8.1f} ns per matrix)")
    for (d, metric, groups), ns in per_matrix.items():
        if d == 64:
            say(f"  per matrix, d = 64 over d = 32, {metric:5s} G={groups:4d}: {ns / per_matrix[32, metric, groups]:.2f}")

if "interval" in parts:
    say(f"interval: three-qubit depolarizing channel, dst='trace', {SHOTS} shots per setting, setup() end to end on the host "
        f"clock, {IREPS} repeats after 1 warm-up")
    np.random.seed(21)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3), dst="trace")
    tmg.experiment(SHOTS, "proj-set")
    tmg.point_estimate("lifp")
    makers = {
        f"BootstrapProcessInterval(n_points={N_POINTS}, method='lifp', sampler='device')":
            lambda: qp.BootstrapProcessInterval(tmg, n_points=N_POINTS, method="lifp", sampler="device", seed=77),
        f"MHMCProcessInterval(n_points={N_POINTS}, burn_steps={BURN})":
            lambda: qp.MHMCProcessInterval(tmg, n_points=N_POINTS, burn_steps=BURN),
    }
    for name, make in makers.items():
        ms = []
        for rep in range(1 + IREPS):
            np.random.seed(5)
            iv = make()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            iv.setup()
            torch.cuda.synchronize()
            if rep:
                ms.append(1e3 * (time.perf_counter() - t0))
        q = iv([0.5, 0.95])[0]
        say(f"  {name}: {stats(ms)}   median / 95 % radius {q[0]:.6f} / {q[1]:.6f}")
