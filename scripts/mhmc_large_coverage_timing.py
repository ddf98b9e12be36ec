#!/usr/bin/env python3
"""The chain coverage study of four- and five-qubit states (quantpy_amd.metrics.get_CL_list_state_mhmc at n = 4, 5) in the
three distances, at the study's defaults n_iter = n_points = burn_steps = 1000, thinning = 1, step 0.01, sampler='device'.
State: the GHZ state mixed half-and-half with the identity; 10 000 (n = 4) / 100 000 (n = 5) shots per setting, at which the
'lin' estimates are positive definite.

  study     the study end to end, per distance: host clock and HIP events around the call, REPS repeats after WARM warm-ups,
            min / median / max.
  fused     the chains alone, Engine.mhmc_state_large_hits on device tensors (no staging): all n_iter chains, per distance;
            and the same chains with no kept state (burn_steps = all steps, n_points = 0) -- the difference is what the
            kept-state distances cost.
  draws     what drawing costs: on --chains chains, the fused kernel without kept states against qt_mhmc_state
            (k_mhmc_state_large) reading increments that qt_mhmc_draws_dim left on the device; and the draws kernel itself.
  unfused   the composition a user had before the fused entry, host pointers as the engine's methods take them, on
            --chains chains in chunks: mhmc_draws_dim -> mhmc_state (the whole chain copied out) -> chol_unparam ->
            hs_dist / metric_dist_dim per chain, the hits counted on the host; host clock, one run, scaled to n_iter chains
            in the report's last column.  The hits are compared with the fused entry's on the same chains.

The report goes to standard output and to `--out`.
Usage: mhmc_large_coverage_timing.py --out PATH [--sizes 4 5] [--chains N4 N5] [--no-unfused] [n_iter [n_points [burn_steps]]]"""
import argparse
import hashlib
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

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--sizes", nargs="*", type=int, default=[4, 5])
ap.add_argument("--chains", nargs=2, type=int, default=[256, 64], help="chains of the draws / unfused blocks at n = 4, 5")
ap.add_argument("--no-unfused", action="store_true")
ap.add_argument("counts", nargs="*", type=int)
opt = ap.parse_args()
N_ITER, N_POINTS, BURN = (opt.counts + [1000, 1000, 1000][len(opt.counts):])[:3]
REPS, WARM = 3, 1
TOTAL = BURN + N_POINTS
SHOTS, STEP, KEY = {4: 10_000, 5: 100_000}, 0.01, 12
CHAINS = dict(zip((4, 5), opt.chains))
CHUNK = {4: 64, 5: 16}  # chains per chunk of the unfused composition (n = 5: 262 MB of increments, as much of chain)
DISTANCES = ("hs", "trace", "if")
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
    """Median (host ms, HIP-event ms)."""
    for _ in range(warm):
        fn()
    t = [timed(fn) for _ in range(reps)]
    say(f"{label}: host {stats([a for a, _ in t])} | HIP events {stats([b for _, b in t])}")
    return float(np.median([a for a, _ in t])), float(np.median([b for _, b in t]))


def mixed_ghz(n):
    d = 2**n
    psi = np.zeros(d, dtype=np.complex128)
    psi[0] = psi[-1] = 1 / np.sqrt(2)
    return 0.5 * np.outer(psi, psi.conj()) + 0.5 * np.eye(d) / d


def study(n, dst):
    return metrics.get_CL_list_state_mhmc(qp.Qobj(mixed_ghz(n)), n_iter=N_ITER, n_points=N_POINTS, n_measurements=SHOTS[n],
                                          step=STEP, burn_steps=BURN, seed=11, dst=dst)


def trials(n):
    """(engine, true state, counts, estimates, x0) of the study's n_iter trials."""
    state = qp.Qobj(mixed_ghz(n))
    tmg = qp.StateTomograph(state, "hs")
    counts = tmg.experiment_batch(SHOTS[n], "proj-set", repeats=N_ITER, sampler="device", seed=11)
    rho, _ = tmg.point_estimate_batch(counts, method="lin")
    eng = tmg._engine()
    x0, status = eng.chol_param(rho)
    assert not status.any()
    return eng, state.matrix, counts, rho, x0


def delta_of(eng, rho, truth, dst):
    return eng.hs_dist(rho, truth) if dst == "hs" else eng.metric_dist_dim(rho, truth, dst)


def fused_block(n, eng, truth, counts, rho, x0):
    """The fused entry on device tensors, all chains: per distance, and without kept states."""
    dev = torch.device("cuda", eng.device)
    on_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (counts, rho, x0)]
    thr = {dst: torch.from_numpy(delta_of(eng, rho, truth, dst)).to(dev) for dst in DISTANCES}
    _, bare = measure(f"n={n} fused chains, no kept state      ",
                      lambda: eng.mhmc_state_large_hits(*on_dev, thr["hs"], KEY, TOTAL, 0, 1, STEP))
    for dst in DISTANCES:
        metric = None if dst == "hs" else dst
        _, full = measure(f"n={n} fused chains, dst={dst:5s}           ",
                          lambda: eng.mhmc_state_large_hits(*on_dev, thr[dst], KEY, BURN, N_POINTS, 1, STEP, metric=metric))
        say(f"n={n} dst={dst:5s}: {N_ITER} chains x {TOTAL} steps, {1e3 * full / TOTAL:.2f} us per step of the launch; the "
            f"{N_POINTS} kept-state distances take {100 * (full - bare) / full:.1f} % of the call (HIP-event medians)")
    return bare


def draws_block(n, eng, counts, x0):
    """On CHAINS[n] chains: the fused kernel without kept states, the unfused kernel on device-resident increments, and
    the draws kernel."""
    c = min(CHAINS[n], N_ITER)
    dev = torch.device("cuda", eng.device)
    d_counts, d_x0 = (torch.from_numpy(np.ascontiguousarray(a[:c])).to(dev) for a in (counts, x0))
    cen = torch.zeros((c, eng.d, eng.d), dtype=torch.complex128, device=dev)
    thr = torch.zeros(c, dtype=torch.float64, device=dev)
    deltas = torch.empty((c, TOTAL, eng.D), dtype=torch.float64, device=dev)
    uniforms = torch.empty((c, TOTAL), dtype=torch.float64, device=dev)
    chain = torch.empty((c, TOTAL, eng.D), dtype=torch.float64, device=dev)
    acc = torch.zeros((c, TOTAL), dtype=torch.int32, device=dev)
    _, t_draw = measure(f"n={n} {c:4d} chains: qt_mhmc_draws_dim       ",
                        lambda: eng.mhmc_draws_dim(eng.D, KEY, c, TOTAL, out=(deltas, uniforms)))

    def unfused_kernel():
        eng._dev_call()
        eng._chk(eng.lib.qt_mhmc_state(eng._h, _ptr(d_counts), c, _ptr(d_x0), _ptr(deltas), _ptr(uniforms), TOTAL, STEP,
                                       _ptr(chain), _ptr(acc), _capi.QT_DEVICE_PTR))

    _, t_read = measure(f"n={n} {c:4d} chains: qt_mhmc_state on them   ", unfused_kernel)
    out = {}

    def fused_kernel():
        out["acc"] = eng.mhmc_state_large_hits(d_counts, cen, d_x0, thr, KEY, 0, 1, TOTAL, STEP)[1]

    # (no burn-in, n_points = 1 with thinning = all steps: one kept state, the first; `accepted` counts every step)
    _, t_self = measure(f"n={n} {c:4d} chains: fused, one kept state   ", fused_kernel)
    same = bool((out["acc"].cpu().numpy() == acc.cpu().numpy().sum(axis=1)).all())
    say(f"n={n} {c:4d} chains x {TOTAL} steps: drawing in the kernel costs {100 * (t_self - t_read) / t_self:.1f} % of the fused "
        f"chain ({1e3 * t_self / TOTAL:.2f} against {1e3 * t_read / TOTAL:.2f} us per step of the launch); the table kernel "
        f"takes {t_draw:.1f} ms for {deltas.numel() * 8 / 2**30:.2f} GiB; accepted steps equal on all chains: {same}")


def unfused_block(n, eng, truth, counts, rho, x0):
    c = min(CHAINS[n], N_ITER)
    deltas_of = {dst: delta_of(eng, rho[:c], truth, dst) for dst in DISTANCES}
    stage = dict(draws=0.0, chain=0.0, unparam=0.0, hs=0.0, trace=0.0)
    stage["if"] = 0.0
    hits = {dst: np.zeros(c, dtype=np.int64) for dst in DISTANCES}

    def lap(name, t0):
        torch.cuda.synchronize()
        stage[name] += time.perf_counter() - t0
        return time.perf_counter()

    for lo in range(0, c, CHUNK[n]):
        hi = min(lo + CHUNK[n], c)
        t = time.perf_counter()
        deltas, uniforms = eng.mhmc_draws_dim(eng.D, KEY, hi - lo, TOTAL, first_chain=lo)
        t = lap("draws", t)
        chain, _ = eng.mhmc_state(counts[lo:hi], x0[lo:hi], deltas, uniforms, STEP)
        t = lap("chain", t)
        kept = np.ascontiguousarray(chain.reshape(hi - lo, TOTAL, eng.D)[:, BURN:][:, :N_POINTS])
        mats = eng.chol_unparam(kept.reshape(-1, eng.D)).reshape(hi - lo, N_POINTS, eng.d, eng.d)
        t = lap("unparam", t)
        for dst in DISTANCES:
            for k in range(lo, hi):
                dist = eng.hs_dist(mats[k - lo], rho[k]) if dst == "hs" else eng.metric_dist_dim(mats[k - lo], rho[k], dst)
                hits[dst][k] = (deltas_of[dst][k] > dist).sum()
            t = lap(dst, t)
    shared = stage["draws"] + stage["chain"] + stage["unparam"]
    say(f"n={n} unfused, {c} chains: draws {stage['draws']:.2f} s, chain {stage['chain']:.2f} s, kept states + unparam "
        f"{stage['unparam']:.2f} s; distances hs {stage['hs']:.2f} s, trace {stage['trace']:.2f} s, if {stage['if']:.2f} s")
    for dst in DISTANCES:
        metric = None if dst == "hs" else dst
        t0 = time.perf_counter()
        got = eng.mhmc_state_large_hits(counts[:c], rho[:c], x0[:c], deltas_of[dst], KEY, BURN, N_POINTS, 1, STEP, metric=metric)[0]
        fused = time.perf_counter() - t0
        total = shared + stage[dst]
        say(f"n={n} dst={dst:5s} {c} chains (host pointers): unfused {total:8.2f} s, fused {1e3 * fused:8.1f} ms = {total / fused:6.0f}x; "
            f"hits equal on {int((got == hits[dst]).sum())} of {c} chains; unfused scaled to {N_ITER} chains: "
            f"{total * N_ITER / c:.0f} s")


with open(_capi.LIB_PATH, "rb") as fh:
    lib_hash = hashlib.sha256(fh.read()).hexdigest()
say(f"library sha256 {lib_hash[:16]}; {torch.cuda.get_device_name(0)}")
say(f"n_iter = {N_ITER}, n_points = {N_POINTS}, burn_steps = {BURN}, thinning = 1, step = {STEP}, sampler = 'device'; {REPS} repeats "
    f"after {WARM} warm-up; host clock and HIP events around each call")
for n in opt.sizes:
    say(f"---- n = {n}: the study end to end ({SHOTS[n]} shots per setting)")
    for dst in DISTANCES:
        measure(f"n={n} dst={dst:5s} study", lambda: study(n, dst))
    eng, truth, counts, rho, x0 = trials(n)
    say(f"---- n = {n}: the fused chains alone (device tensors)")
    fused_block(n, eng, truth, counts, rho, x0)
    say(f"---- n = {n}: what the draws cost")
    draws_block(n, eng, counts, x0)
    if not opt.no_unfused:
        say(f"---- n = {n}: the unfused composition")
        unfused_block(n, eng, truth, counts, rho, x0)
report.close()
