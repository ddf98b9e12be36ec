#!/usr/bin/env python3
"""The 'states' process estimator end to end, on a tree with the batched device path (qt_states_choi_batch) and on its
parent, whose point_estimate_batch(method='states') assembles on the host and tests every trial with Channel.is_cptp.

  estimator  `ProcessTomograph.point_estimate_batch(counts, method='states')` on B = 1000 experiments of a depolarizing
             channel (p = 0.1 at n = 1, 3; p = 0.6 at n = 2, where most trials need the projection), output states by
             'lin' at n = 1, 2, 3 and by 'mle' at n = 1, 2.
  interval   `BootstrapProcessInterval(method='states', n_points=1000).setup()` at n = 2.
  study      the bootstrap coverage study with n_iter = n_points = 1000 at n = 1, 2.  With the device path:
             `metrics.get_CL_list_channel_boot_states`.  Without it (and, for comparison, with it): the ungrouped
             composition -- per trial, `device_multinomial` of its n_points resamples, point_estimate_batch(method='states'),
             `Engine.distance`, a strict count -- on the first TRIALS trials, reported per trial beside the study's time per
             trial.
  kernels    (device path only) HIP events on the engine's stream around the assembly (`states_choi_dev(cptp=False)`), the
             test (`is_cptp` on device tensors) and the projection of the failing trials (qt_cptp_project_batch on device
             pointers), B = 1000 matrices resident on the device, at n = 1, 2, 3.

Host clock after one warm-up, REPS repeats, median (min - max).  The report goes to standard output and is APPENDED to
`--out` (default profiles/states_estimator_timing.txt), so that runs of the two trees can alternate into one file.
Usage: states_estimator_timing.py [--out PATH] [--label TEXT] [estimator] [interval] [study] [kernels]"""
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi, metrics  # noqa: E402

B, SHOTS, REPS, N_POINTS, N_ITER, TRIALS = 1000, 1000, 5, 1000, 1000, 10
NOISE = {1: 0.1, 2: 0.6, 3: 0.1}
args = sys.argv[1:]
out_path, label = os.path.join(ROOT, "profiles", "states_estimator_timing.txt"), "this tree"
while args[:1] and args[0] in ("--out", "--label"):
    if args[0] == "--out":
        out_path = args[1]
    else:
        label = args[1]
    args = args[2:]
parts = args or ["estimator", "interval", "study", "kernels"]
report = open(out_path, "a")
HAVE = "qt_states_choi_batch" in _capi.SIGNATURES


def say(line):
    print(line, flush=True)
    report.write(line + "\n")
    report.flush()


def stats(ms):
    ms = np.asarray(ms)
    return f"median {np.median(ms):10.3f}  ({ms.min():10.3f} - {ms.max():10.3f}) ms"


def host_clock(fn, reps=REPS):
    ms = []
    for rep in range(1 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            ms.append(1e3 * (time.perf_counter() - t0))
    return ms, out


def tomograph(n, repeats):
    np.random.seed(30 + n)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(NOISE[n], n), input_states="proj4")
    return tmg, tmg.experiment_batch(SHOTS, "proj-set", repeats=repeats)


say(f"[{label}] batched device path of the 'states' estimator: {HAVE}")
if "estimator" in parts:
    say(f"estimator: point_estimate_batch(method='states'), B = {B}, {SHOTS} shots, host clock, {REPS} repeats after 1 warm-up")
    for n, method in ((1, "lin"), (1, "mle"), (2, "lin"), (2, "mle"), (3, "lin")):
        tmg, counts = tomograph(n, B)
        ms, choi = host_clock(lambda: tmg.point_estimate_batch(counts, method="states", states_est_method=method))
        say(f"  n={n} {method}: {stats(ms)}   checksum {np.abs(choi).sum():.9f}")

if "interval" in parts:
    say(f"interval: BootstrapProcessInterval(method='states', n_points={N_POINTS}).setup() at n = 2, host clock, "
        f"{REPS} repeats after 1 warm-up")
    tmg, _ = tomograph(2, 1)
    tmg.point_estimate("states")

    def run():
        np.random.seed(5)
        iv = qp.BootstrapProcessInterval(tmg, n_points=N_POINTS, method="states")
        iv.setup()
        return iv

    ms, iv = host_clock(run)
    q = iv([0.5, 0.95])[0]
    say(f"  n=2: {stats(ms)}   median / 95 % radius {q[0]:.6f} / {q[1]:.6f}")

if "study" in parts:
    say(f"study: n_iter = n_points = {N_ITER}, {SHOTS} shots; the ungrouped composition on the first {TRIALS} trials")
    for n in (1, 2):
        channel = qp.channel.depolarizing(0.1, n)
        seed = 900 + n
        tmg = qp.ProcessTomograph(channel, "proj4", "hs")
        counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=N_ITER, sampler="device", seed=seed)
        estimates = tmg.point_estimate_batch(counts, method="lifp")
        eng = tmg._engine()
        delta = eng.distance(estimates, channel.choi.matrix)
        pvals = eng.process_born_probs(estimates)
        dd, s, k = eng.D, eng.S, eng.K
        shots = np.tile(np.full(s, SHOTS, dtype=np.int64), dd)

        def composition():
            hits = np.zeros(TRIALS, dtype=np.int64)
            for t in range(TRIALS):
                resamples = np.stack([eng.device_multinomial(shots, pvals[t].reshape(dd * s, k), dd * s, seed + 1,
                                                             first_row=(r * N_ITER + t) * dd * s).reshape(dd, s, k)
                                      for r in range(N_POINTS)])
                dist = eng.distance(tmg.point_estimate_batch(resamples, method="states"), estimates[t])
                hits[t] = (delta[t] > dist).sum()
            return hits

        ms, hits = host_clock(composition, reps=2)
        say(f"  n={n} ungrouped composition, per trial: {stats(np.asarray(ms) / TRIALS)}   hits {hits.tolist()}")
        if HAVE:
            ms, out = host_clock(lambda: metrics.get_CL_list_channel_boot_states(
                channel, n_iter=N_ITER, n_points=N_POINTS, n_measurements=SHOTS, seed=seed, return_details=True), reps=3)
            say(f"  n={n} get_CL_list_channel_boot_states, whole study: {stats(ms)}")
            say(f"  n={n} get_CL_list_channel_boot_states, per trial:   {stats(np.asarray(ms) / N_ITER)}   "
                f"hits {out['hits'][:TRIALS].tolist()}")

if "kernels" in parts and HAVE:
    say(f"kernels: B = {B} matrices on the device, HIP events on the engine's stream, {REPS} repeats after 1 warm-up")
    for n in (1, 2, 3):
        tmg, counts = tomograph(n, B)
        eng = tmg._engine()
        outs = eng.lin(counts.reshape((-1,) + counts.shape[2:]))
        states = torch.from_numpy(outs.reshape(B, eng.D, eng.d, eng.d)).cuda()
        w = torch.from_numpy(tmg._states_weights()).cuda()
        choi = torch.empty((B, eng.D, eng.D), dtype=torch.complex128, device="cuda")

        def events(fn):
            ms = []
            for rep in range(1 + REPS):
                eng.sync()
                eng.timer_begin()
                fn()
                t = eng.timer_end()
                if rep:
                    ms.append(t)
            return ms

        say(f"  n={n} assembly:   {stats(events(lambda: eng.states_choi_dev(states, w, choi, cptp=False)))}")
        ok = eng.is_cptp(choi)
        eng.sync()
        failing = choi[ok == 0].contiguous()
        say(f"  n={n} test:       {stats(events(lambda: eng.is_cptp(choi)))}")
        if len(failing):
            proj = torch.empty_like(failing)
            iters = torch.empty(len(failing), dtype=torch.int32, device="cuda")
            call = lambda: eng._chk(eng.lib.qt_cptp_project_batch(  # noqa: E731
                eng._h, ctypes.c_void_p(failing.data_ptr()), len(failing), 0, 1000, 1e-12, ctypes.c_void_p(proj.data_ptr()),
                ctypes.c_void_p(iters.data_ptr()), _capi.QT_DEVICE_PTR))
            say(f"  n={n} projection of the {len(failing)} failing trials: {stats(events(call))}")
        else:
            say(f"  n={n} projection: no trial of the batch fails the test")
        say(f"  n={n} whole call (assembly, test, read-back, projection): "
            f"{stats(events(lambda: eng.states_choi_dev(states, w, choi, cptp=True)))}")
