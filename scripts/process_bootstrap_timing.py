#!/usr/bin/env python3
"""BootstrapProcessInterval on a two-qubit depolarizing channel at 1000 shots ('proj-set', 'proj4' inputs), and the
kernels under it:

  * `BootstrapProcessInterval(tmg, n_points)(levels)` for both samplers: end-to-end (host clock, the call ends in a device
    synchronise) and GPU time (HIP events on torch's current stream around the call: the span from the first to the last
    piece of device work, host gaps between them included);
  * the reconstruction alone on device-resident counts: `lifp_dist_dev` (one pass, no matrices stored) against
    `lifp_dev` + the Hilbert-Schmidt distance kernel on the stored matrices (two passes), HIP events around each.

Every figure is min / median / max over REPS warm repeats.  The script runs on any commit: where the engine has no
`lifp_dist_dev` only the two-pass form is timed.  Usage: process_bootstrap_timing.py [n_points ...] (default 2000 131072)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi  # noqa: E402

REPS, WARM = 7, 2
LEVELS = np.array([0.5, 0.9, 0.95])


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


def repeat(fn):
    for _ in range(WARM):
        fn()
    out = np.array([timed(fn) for _ in range(REPS)])
    return out[:, 0], out[:, 1]


np.random.seed(7)
tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 2))
tmg.experiment(1000, "proj-set")
tmg.point_estimate("lifp")
eng = tmg._engine()
fused = hasattr(eng, "lifp_dist_dev")
print(f"one-pass entry (lifp_dist_dev): {'yes' if fused else 'no'};  {REPS} repeats after {WARM} warm-up calls", flush=True)

for n_points in [int(a) for a in sys.argv[1:]] or [2000, 131072]:
    for sampler in ("numpy", "device"):
        def interval():
            np.random.seed(4242)
            iv = qp.BootstrapProcessInterval(tmg, n_points=n_points, sampler=sampler, seed=None if sampler == "numpy" else 5)
            interval.radii = iv(LEVELS)[0]

        host, gpu = repeat(interval)
        print(f"interval n_points={n_points:7d} sampler={sampler:6s}: end-to-end {stats(host)} | HIP events {stats(gpu)} | "
              f"radii {interval.radii}", flush=True)

boot = qp.ProcessTomograph(tmg.reconstructed_channel, tmg.input_states, tmg.dst)
first = tmg.tomographs[0]
centre = torch.from_numpy(np.ascontiguousarray(tmg.reconstructed_channel.choi.matrix, dtype=np.complex128)).cuda()
for b in (1024, 65536):
    counts = torch.from_numpy(boot.experiment_batch(first.n_measurements, povm=first.povm_matrix, repeats=b, sampler="device",
                                                    seed=3)).cuda()
    eng = boot._engine()
    choi = torch.empty((b, 16, 16), dtype=torch.complex128, device="cuda")
    d2 = torch.empty(b, dtype=torch.float64, device="cuda")
    d1 = torch.empty(b, dtype=torch.float64, device="cuda")
    for cptp in (True, False):
        def two_pass():
            eng.lifp_dev(counts, choi, cptp=cptp)
            eng._chk(eng.lib.qt_hs_dist_dim(eng._h, 16, choi.data_ptr(), centre.data_ptr(), b, d2.data_ptr(), _capi.QT_DEVICE_PTR))

        def one_pass():
            eng.lifp_dist_dev(counts, centre, d1, cptp=cptp)

        # alternate the two forms so that whatever else runs on the machine meets both alike
        rows = {"two passes (lifp_dev + hs_dist)": two_pass}
        if fused:
            rows["one pass   (lifp_dist_dev)     "] = one_pass
        for fn in rows.values():
            for _ in range(WARM):
                fn()
        ms = {name: [] for name in rows}
        for _ in range(REPS):
            for name, fn in rows.items():
                ms[name].append(timed(fn)[1])
        for name in rows:
            print(f"B={b:6d} cptp={int(cptp)} {name}: HIP events {stats(ms[name])}", flush=True)
        if fused:
            print(f"B={b:6d} cptp={int(cptp)} max |one pass - two passes| = {float((d1 - d2).abs().max()):.3e}", flush=True)
