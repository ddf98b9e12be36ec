#!/usr/bin/env python3
"""The bootstrap coverage study for processes (quantpy_amd.metrics.get_CL_list_channel_boot) on depolarizing(0.1, n) at
1000 shots per setting ('proj-set', 'proj4' inputs):

  * per chunk of whole resamples, n = 1, 2, 3, cptp on and off, HIP events and host clock, warm, the two forms alternating
    in one process on the SAME device-resident counts:
      grouped    ONE qt_lifp_dist_group_batch over the chunk's R x n_iter resamples (resample-major) + qt_group_hits
      per trial  n_iter calls of the ungrouped qt_lifp_dist_batch, one per trial, on that trial's R resamples (a trial-major
                 copy of the same counts, made outside the timed region), each against its own centre
    and the sampler call that fills the chunk, which both forms share; max |difference| of the two forms' distances;
  * end to end at n = 2, n_iter = n_points = 1000: the call itself, host clock (it ends in a device synchronise): trial
    counts, point estimates, the table of qt_process_born_probs, every chunk, the hits back.

Every figure is min / median / max over REPS warm repeats.  The report goes to standard output and to `--out`
(default profiles/process_bootstrap_coverage_timing.txt).
Usage: process_bootstrap_coverage_timing.py [--out PATH] [n_iter_n1 n_iter_n2 n_iter_n3 [n_points]]  (default 1000 1000 100 1000)"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import metrics  # noqa: E402

REPS, WARM = 5, 1
SHOTS = 1000
args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "process_bootstrap_coverage_timing.txt")
if args[:1] == ["--out"]:
    out_path, args = args[1], args[2:]
N_ITER = dict(zip((1, 2, 3), [int(a) for a in args[:3]])) if len(args) >= 3 else {1: 1000, 2: 1000, 3: 100}
N_POINTS = int(args[3]) if len(args) > 3 else 1000
report = open(out_path, "w")


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


def stats(ms):
    ms = np.asarray(ms)
    return f"min {ms.min():9.3f}  median {np.median(ms):9.3f}  max {ms.max():9.3f} ms"


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


say(f"depolarizing(0.1, n), {SHOTS} shots per setting, n_points = {N_POINTS}; {REPS} repeats after {WARM} warm-up")

# ---- one chunk, grouped against per trial ---------------------------------------------------------------------------------
for n in (1, 2, 3):
    n_iter = N_ITER[n]
    channel = qp.channel.depolarizing(0.1, n)
    out = metrics.get_CL_list_channel_boot(channel, n_iter=n_iter, n_points=1, n_measurements=SHOTS, seed=11, return_details=True)
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    tmg.experiment_batch(SHOTS, "proj-set", repeats=1, sampler="device", seed=11)  # registers the POVM and the shots
    eng = tmg._engine()
    dd, n_set, n_out = eng.D, eng.S, eng.K
    per = dd * n_set  # table rows per process
    rows = max(1, min(N_POINTS, metrics._CHUNK_BYTES // (n_iter * per * n_out * 8)))  # the study's default chunk
    b = rows * n_iter
    choi, delta = out["estimates"], out["delta"]
    centres = torch.from_numpy(np.ascontiguousarray(choi)).cuda()
    p_d = eng.process_born_probs(centres).view(n_iter * per, n_out)
    n_d = torch.from_numpy(np.tile(np.full(n_set, SHOTS, dtype=np.int64), n_iter * dd)).cuda()
    thr = torch.from_numpy(np.ascontiguousarray(delta)).cuda()
    counts = torch.empty((b, dd, n_set, n_out), dtype=torch.int64, device="cuda")
    dist_g = torch.empty(b, dtype=torch.float64, device="cuda")
    dist_t = torch.empty((n_iter, rows), dtype=torch.float64, device="cuda")
    hits = torch.zeros(n_iter, dtype=torch.int64, device="cuda")
    status = torch.zeros(b, dtype=torch.int32, device="cuda")

    def sample():
        eng.device_multinomial(n_d, p_d, b * per, out["seed"], first_row=0, out=counts)

    def table():
        eng.process_born_probs(centres, out=p_d)

    sample()
    torch.cuda.synchronize()
    by_trial = counts.view(rows, n_iter, dd, n_set, n_out).transpose(0, 1).contiguous()  # [trial][resample]
    say(f"n={n}: chunk of {rows} resamples x {n_iter} trials = {b} reconstructions, {counts.numel() * 8 / 2**20:.0f} MB of counts")
    say(f"n={n} qt_process_born_probs of {n_iter} estimates: HIP events {stats([timed(table)[1] for _ in range(REPS)])}")
    say(f"n={n} sampler (both forms): HIP events {stats([timed(sample)[1] for _ in range(REPS)])}")
    for cptp in (True, False):
        def grouped():
            eng.lifp_dist_dev(counts, centres, dist_g, cptp=cptp, status=status)
            eng.group_hits(dist_g, thr, hits)

        def per_trial():
            st = status.view(n_iter, rows)
            for t in range(n_iter):
                eng.lifp_dist_dev(by_trial[t], centres[t], dist_t[t], cptp=cptp, status=st[t])

        forms = {"grouped  ": grouped, "per trial": per_trial}
        for fn in forms.values():
            for _ in range(WARM):
                fn()
        res = {name: [] for name in forms}
        for _ in range(REPS):  # alternating, so that whatever else runs on the machine meets both alike
            for name, fn in forms.items():
                res[name].append(timed(fn))
        for name in forms:
            r = np.array(res[name])
            say(f"n={n} cptp={int(cptp)} chunk {name}: HIP events {stats(r[:, 1])} | host {stats(r[:, 0])}")
        diff = float((dist_g.view(rows, n_iter).t() - dist_t).abs().max())
        say(f"n={n} cptp={int(cptp)} chunk: max |grouped - per trial| = {diff:.3e}")
    del counts, by_trial

# ---- end to end ---------------------------------------------------------------------------------------------------------------
channel = qp.channel.depolarizing(0.1, 2)
for cptp in (True, False):
    def study():
        study.levels = metrics.get_CL_list_channel_boot(channel, n_iter=N_ITER[2], n_points=N_POINTS, n_measurements=SHOTS,
                                                        cptp=cptp, seed=11)

    for _ in range(WARM):
        study()
    host = [timed(study)[0] for _ in range(REPS)]
    lv = study.levels
    say(f"end to end n=2 n_iter={N_ITER[2]} n_points={N_POINTS} cptp={int(cptp)}: {stats(host)} | "
        f"{N_ITER[2] * N_POINTS / np.median(host) * 1e-3:.2f} M resamples/s | levels: mean {lv.mean():.3f}, "
        f"share below 0.9: {(lv < 0.9).mean():.3f}")
report.close()
