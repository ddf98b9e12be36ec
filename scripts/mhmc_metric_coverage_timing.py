#!/usr/bin/env python3
"""The chain coverage studies in trace distance and infidelity (quantpy_amd.metrics.get_CL_list_state_mhmc /
get_CL_list_channel_mhmc with dst=...) and the process bootstrap study in trace distance, at the studies' defaults
n_iter = n_points = burn_steps = 1000, thinning = 1, sampler='device'.

  study     the study end to end, per distance: host clock and HIP events around the call, REPS repeats after WARM warm-ups,
            min / median / max.  States: the GHZ state mixed half-and-half with the identity, 1000 shots per setting, n = 1,
            2, 3, step 0.01.  Channels: depolarizing(0.2), 2000 shots, n = 1, 2, steps 0.006 / 0.0006.
  unfused   the same chains on entries that predate the fused kernels, in chunks: qt_mhmc_draws / qt_mhmc_process_draws,
            qt_mhmc_state / qt_mhmc_process (the whole chain copied out), qt_chol_unparam (states), the metric of the kept
            states by qt_metric_dist_group_batch / qt_metric_dist_dim per chain, the hits counted on the host; host clock.
  boot      get_CL_list_channel_boot at n = 2, n_iter = n_points = 1000, against get_CL_list_channel_boot_dst(dst='trace').

A tree whose studies have no `dst` argument (the parent of the change that added it) runs the 'hs' studies alone: that is
the baseline the 'hs' lines of this tree are held against.  --repeat-hs N runs the 'hs' block N times over, for the
run-to-run spread.  The report goes to standard output and to `--out`.
Usage: mhmc_metric_coverage_timing.py --out PATH [--repeat-hs N] [--no-unfused] [--no-boot] [n_iter [n_points [burn_steps]]]"""
import argparse
import hashlib
import inspect
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi, metrics  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--repeat-hs", type=int, default=1)
ap.add_argument("--no-unfused", action="store_true")
ap.add_argument("--no-boot", action="store_true")
ap.add_argument("sizes", nargs="*", type=int)
opt = ap.parse_args()
N_ITER, N_POINTS, BURN = (opt.sizes + [1000, 1000, 1000][len(opt.sizes):])[:3]
REPS, WARM = 3, 1
TOTAL = BURN + N_POINTS
STATE_SHOTS, STATE_STEP = 1000, 0.01
PROC_SHOTS, PROC_STEPS = 2000, {1: 0.006, 2: 0.0006}
STATE_CHUNK = 100               # chains per chunk of the unfused composition (n = 3: 102 MB of increments, as much of chain)
PROC_CHUNK = {1: 250, 2: 50}    # (n = 2: 205 MB of increments, 410 MB of chain)
HAS_DST = "dst" in inspect.signature(metrics.get_CL_list_state_mhmc).parameters
report = open(opt.out, "w")


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


def measure(label, fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    t = [timed(fn) for _ in range(reps)]
    say(f"{label}: host {stats([a for a, _ in t])} | HIP events {stats([b for _, b in t])}")
    return float(np.median([a for a, _ in t]))


def mixed_ghz(n):
    d = 2**n
    psi = np.zeros(d, dtype=np.complex128)
    psi[0] = psi[-1] = 1 / np.sqrt(2)
    return 0.5 * np.outer(psi, psi.conj()) + 0.5 * np.eye(d) / d


def state_study(n, dst):
    kw = dict(dst=dst) if HAS_DST else {}
    return metrics.get_CL_list_state_mhmc(qp.Qobj(mixed_ghz(n)), n_iter=N_ITER, n_points=N_POINTS, n_measurements=STATE_SHOTS,
                                          step=STATE_STEP, burn_steps=BURN, seed=11, **kw)


def channel_study(n, dst):
    kw = dict(dst=dst) if HAS_DST else {}
    return metrics.get_CL_list_channel_mhmc(qp.channel.depolarizing(0.2, n), n_iter=N_ITER, n_points=N_POINTS,
                                            n_measurements=PROC_SHOTS, step=PROC_STEPS[n], burn_steps=BURN, seed=11, **kw)


def boot_study(dst):
    study = metrics.get_CL_list_channel_boot if dst == "hs" else lambda *a, **k: metrics.get_CL_list_channel_boot_dst(*a, dst=dst, **k)
    return study(qp.channel.depolarizing(0.2, 2), n_iter=N_ITER, n_points=N_POINTS, n_measurements=PROC_SHOTS, seed=11)


def state_unfused(n, metric):
    state = qp.Qobj(mixed_ghz(n))
    tmg = qp.StateTomograph(state, "hs")
    counts = tmg.experiment_batch(STATE_SHOTS, "proj-set", repeats=N_ITER, sampler="device", seed=11)
    rho, _ = tmg.point_estimate_batch(counts, method="lin")
    eng = tmg._engine()
    delta = eng.metric_dist(rho, state.matrix, metric)
    x0, status = eng.chol_param(rho)
    assert not status.any()
    out = {}

    def run():
        hits = np.zeros(N_ITER, dtype=np.int64)
        for lo in range(0, N_ITER, STATE_CHUNK):
            hi = min(lo + STATE_CHUNK, N_ITER)
            deltas, uniforms = eng.mhmc_draws(12, hi - lo, TOTAL, first_chain=lo)
            chain, _ = eng.mhmc_state(counts[lo:hi], x0[lo:hi], deltas, uniforms, STATE_STEP)
            kept = np.ascontiguousarray(chain[:, BURN:][:, :N_POINTS])
            mats = eng.chol_unparam(kept.reshape(-1, eng.D)).reshape(hi - lo, N_POINTS, eng.d, eng.d)
            for c in range(lo, hi):
                hits[c] = (delta[c] > eng.metric_dist(mats[c - lo], rho[c], metric)).sum()
        out["hits"] = hits

    def fused():
        out["fused"] = eng.mhmc_state_hits(counts, rho, x0, delta, 12, BURN, N_POINTS, 1, STATE_STEP, metric=metric)[0]

    return run, fused, out


def channel_unfused(n, metric):
    channel = qp.channel.depolarizing(0.2, n)
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(PROC_SHOTS, "proj-set", repeats=N_ITER, sampler="device", seed=11)
    choi = tmg.point_estimate_batch(counts, method="lifp")
    eng = tmg._engine()
    delta = eng.metric_dist_dim(choi, channel.choi.matrix, metric)
    out = {}

    def run():
        hits = np.zeros(N_ITER, dtype=np.int64)
        for lo in range(0, N_ITER, PROC_CHUNK[n]):
            hi = min(lo + PROC_CHUNK[n], N_ITER)
            deltas, uniforms = eng.mhmc_process_draws(12, hi - lo, TOTAL, first_chain=lo)
            chain, _ = eng.mhmc_process(counts[lo:hi], choi[lo:hi], deltas, uniforms, PROC_STEPS[n])
            kept = np.ascontiguousarray(chain[:, BURN:][:, :N_POINTS].real)
            for c in range(lo, hi):
                hits[c] = (delta[c] > eng.metric_dist_dim(kept[c - lo], choi[c], metric)).sum()
        out["hits"] = hits

    def fused():
        out["fused"] = eng.mhmc_process_hits(counts, choi, choi, delta, 12, BURN, N_POINTS, 1, PROC_STEPS[n], metric=metric)[0]

    return run, fused, out


with open(_capi.LIB_PATH, "rb") as fh:
    lib_hash = hashlib.sha256(fh.read()).hexdigest()
say(f"library sha256 {lib_hash[:16]}; studies take dst: {HAS_DST}; {torch.cuda.get_device_name(0)}")
say(f"n_iter = {N_ITER}, n_points = {N_POINTS}, burn_steps = {BURN}, thinning = 1, sampler = 'device'; {REPS} repeats after {WARM} "
    f"warm-up; host clock and HIP events around each call")

for rnd in range(opt.repeat_hs):
    say(f"---- 'hs' studies, round {rnd + 1} of {opt.repeat_hs}")
    for n in (1, 2, 3):
        measure(f"state   n={n} dst=hs    study", lambda: state_study(n, "hs"))
    for n in (1, 2):
        measure(f"channel n={n} dst=hs    study", lambda: channel_study(n, "hs"))
if not opt.no_boot:
    measure("channel boot n=2 dst=hs    study", lambda: boot_study("hs"), reps=2)
if HAS_DST:
    say("---- the new distances")
    for n in (1, 2, 3):
        for dst in ("trace", "if"):
            measure(f"state   n={n} dst={dst:5s} study", lambda: state_study(n, dst))
    for n in (1, 2):
        measure(f"channel n={n} dst=trace study", lambda: channel_study(n, "trace"))
    if not opt.no_boot:
        measure("channel boot n=2 dst=trace study", lambda: boot_study("trace"), reps=2)
    if not opt.no_unfused:
        say("---- the chains alone (host-pointer calls): the fused entry against the unfused composition")
        jobs = [("state  ", n, m, state_unfused) for n in (1, 2, 3) for m in ("trace", "if")]
        jobs += [("channel", n, "trace", channel_unfused) for n in (1, 2)]
        for kind, n, metric, make in jobs:
            run, fused, out = make(n, metric)
            slow = kind == "channel" and n == 2
            a = measure(f"{kind} n={n} {metric:5s} chains fused  ", fused)
            b = measure(f"{kind} n={n} {metric:5s} chains unfused", run, reps=1 if slow else REPS, warm=0 if slow else WARM)
            say(f"{kind} n={n} {metric:5s} chains: unfused / fused = {b / a:.1f}x (medians); hits equal on "
                f"{int((out['hits'] == out['fused']).sum())} of {N_ITER} chains")
report.close()
