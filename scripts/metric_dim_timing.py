#!/usr/bin/env python3
"""Trace distance and infidelity of 16 x 16 and 32 x 32 matrices on the engine (qt_metric_dist_dim) and the bootstrap
interval built on them.

  kernel    `Engine.metric_dist_dim_dev` on random full-rank density matrices resident on the device, 65 536 of them at
            d = 16 and 16 384 at d = 32, both metrics, against one centre (G = 1) and against a table of G = 1000 centres;
            HIP events on the engine's stream, REPS repeats after WARM warm-ups, median (min - max).  The infidelity
            includes its set-up launch (k_psd_sqrt_dim of the G centres).
  interval  `BootstrapStateInterval(n_points=2000, method='mle', sampler='device').setup()` at n = 4 and n = 5 with
            dst='trace' and dst='if', end to end on the host clock (counts drawn on the device, the reconstructions, the
            distances, the sorted sample), IREPS repeats after one warm-up, median (min - max).

A tree without `Engine.metric_dist_dim` (the parent of the change that added it) runs `interval` alone: there the distances
are one scipy.linalg.sqrtm loop per resample on the host, and that is the baseline.  The report goes to standard output and
is APPENDED to `--out` (default profiles/metric_dim_timing.txt), so that runs of the two trees can alternate into one file.
Usage: metric_dim_timing.py [--out PATH] [--label TEXT] [kernel] [interval]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402

BATCH, TABLE = {16: 65536, 32: 16384}, 1000
REPS, WARM = 20, 3
IREPS, N_POINTS, SHOTS = 3, 2000, 1000
args = sys.argv[1:]
out_path, label = os.path.join(ROOT, "profiles", "metric_dim_timing.txt"), "this tree"
while args[:1] and args[0] in ("--out", "--label"):
    if args[0] == "--out":
        out_path = args[1]
    else:
        label = args[1]
    args = args[2:]
parts = args or ["kernel", "interval"]
report = open(out_path, "a")
HAVE = hasattr(qp.engine.Engine, "metric_dist_dim")


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


say(f"[{label}] distances of 16 x 16 and 32 x 32 matrices on the engine: {HAVE}")
if "kernel" in parts and HAVE:
    say(f"kernel: metric_dist_dim_dev, matrices on the device, HIP events, {REPS} repeats after {WARM} warm-ups")
    eng = qp.get_engine(5)
    for d in (16, 32):
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
                    eng.metric_dist_dim_dev(rho, centres, dist, metric)
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= WARM:
                        ms.append(e0.elapsed_time(e1))
                groups = centres.shape[0] if centres.dim() == 3 else 1
                say(f"  d={d} B={b} {metric:5s} G={groups:4d}: {stats(ms)}   ({1e6 * np.median(ms) / b:8.1f} ns per matrix)")

if "interval" in parts:
    say(f"interval: BootstrapStateInterval(n_points={N_POINTS}, method='mle', sampler='device'), {SHOTS} shots per setting, "
        f"setup() end to end on the host clock, {IREPS} repeats after 1 warm-up")
    for n in (4, 5):
        state = qp.Qobj(full_rank(np.random.default_rng(8 + n), 1, 2**n)[0])
        for dst in ("trace", "if"):
            np.random.seed(21)
            tmg = qp.StateTomograph(state, dst)
            tmg.experiment(SHOTS, "proj-set")
            tmg.point_estimate("mle")
            ms = []
            for rep in range(1 + IREPS):
                iv = qp.BootstrapStateInterval(tmg, n_points=N_POINTS, method="mle", sampler="device", seed=77)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                iv.setup()
                torch.cuda.synchronize()
                if rep:
                    ms.append(1e3 * (time.perf_counter() - t0))
            q = iv([0.5, 0.95])[0]
            say(f"  n={n} dst={dst:5s}: {stats(ms)}   one-pass: {hasattr(iv, 'sample')}   median / 95 % radius "
                f"{q[0]:.6f} / {q[1]:.6f}")
