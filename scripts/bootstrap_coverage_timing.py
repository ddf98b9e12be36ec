#!/usr/bin/env python3
"""The bootstrap coverage study (quantpy_amd.metrics.get_CL_list_state, interval='boot') on GHZ at n = 3, 1000 shots per
setting, n_iter = n_points = 1000, method_boot 'lin' and 'mle':

  * end to end: the call itself, host clock (it ends in a device synchronise): trial counts, point estimates, Born
    probabilities, every chunk, the hits back;
  * per chunk, HIP events and host clock, warm, the two forms alternating in one process on the SAME device-resident counts:
      grouped    ONE qt_*_dist_group_batch over the chunk's R x n_iter resamples (resample-major) + qt_group_hits
      per trial  n_iter calls of the ungrouped qt_*_dist_batch, one per trial, on that trial's R resamples (a trial-major
                 copy of the same counts, made outside the timed region), each against its own centre
    and the sampler call that fills the chunk, which both forms share;
  * max |difference| of the two forms' distances (they are the same bits).

Every figure is min / median / max over REPS warm repeats.  Usage: bootstrap_coverage_timing.py [n_iter [n_points]]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import metrics  # noqa: E402

REPS, WARM = 5, 1
N_ITER = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
N_POINTS = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
SHOTS = 1000


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


state = qp.qobj.GHZ(3)
print(f"GHZ(3), {SHOTS} shots per setting, n_iter = {N_ITER}, n_points = {N_POINTS}; {REPS} repeats after {WARM} warm-up", flush=True)

for method_boot in ("lin", "mle"):
    def study():
        study.levels = metrics.get_CL_list_state(state, n_iter=N_ITER, n_points=N_POINTS, interval="boot",
                                                 n_measurements=SHOTS, method_boot=method_boot, seed=11)

    for _ in range(WARM):
        study()
    host = [timed(study)[0] for _ in range(REPS)]
    lv = study.levels
    print(f"end to end  method_boot={method_boot}: {stats(host)} | {N_ITER * N_POINTS / np.median(host) * 1e-3:.2f} M resamples/s | "
          f"levels: mean {lv.mean():.3f}, share below 0.9: {(lv < 0.9).mean():.3f}", flush=True)

# ---- one chunk, grouped against per trial ---------------------------------------------------------------------------------
out = metrics.get_CL_list_state(state, n_iter=N_ITER, n_points=1, interval="boot", n_measurements=SHOTS, seed=11,
                                return_details=True)
tmg = qp.StateTomograph(state)
tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", 3)
tmg.n_measurements = np.ones(tmg.povm_matrix.shape[0]) * SHOTS
eng = tmg._engine()
n_set, n_out = eng.S, eng.K
rows = max(1, min(N_POINTS, metrics._CHUNK_BYTES // (N_ITER * n_set * n_out * 8)))  # the study's default chunk
b = rows * N_ITER
rho, delta = out["estimates"], out["delta"]
pvals = np.clip(eng.born_probs(eng.bloch_from_matrix(rho)), 0, 1).reshape(N_ITER * n_set, n_out)
p_d = torch.from_numpy(pvals).cuda()
n_d = torch.from_numpy(np.tile(np.full(n_set, SHOTS, dtype=np.int64), N_ITER)).cuda()
centres = torch.from_numpy(np.ascontiguousarray(rho)).cuda()
thr = torch.from_numpy(np.ascontiguousarray(delta)).cuda()
counts = torch.empty((b, n_set, n_out), dtype=torch.int64, device="cuda")
dist_g = torch.empty(b, dtype=torch.float64, device="cuda")
dist_t = torch.empty((N_ITER, rows), dtype=torch.float64, device="cuda")
hits = torch.zeros(N_ITER, dtype=torch.int64, device="cuda")
status = torch.zeros(b, dtype=torch.int32, device="cuda")


def sample():
    eng.device_multinomial(n_d, p_d, b * n_set, out["seed"], first_row=0, out=counts)


sample()
torch.cuda.synchronize()
by_trial = counts.view(rows, N_ITER, n_set, n_out).transpose(0, 1).contiguous()  # [trial][resample]: the per-trial calls' input
print(f"chunk: {rows} resamples x {N_ITER} trials = {b} reconstructions, {counts.numel() * 8 / 2**20:.0f} MB of counts", flush=True)
ms = [timed(sample)[1] for _ in range(REPS)]
print(f"sampler (both forms): HIP events {stats(ms)}", flush=True)

for method_boot in ("lin", "mle"):
    def grouped():
        if method_boot == "lin":
            eng.lin_dist_dev(counts, centres, dist_g, status=status)
        else:
            eng.mle_dist_dev(counts, centres, dist_g, status=status)
        eng.group_hits(dist_g, thr, hits)

    def per_trial():
        st = status.view(N_ITER, rows)
        for t in range(N_ITER):
            if method_boot == "lin":
                eng.lin_dist_dev(by_trial[t], centres[t], dist_t[t], status=st[t])
            else:
                eng.mle_dist_dev(by_trial[t], centres[t], dist_t[t], status=st[t])

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
        print(f"chunk method_boot={method_boot} {name}: HIP events {stats(r[:, 1])} | host {stats(r[:, 0])}", flush=True)
    diff = float((dist_g.view(rows, N_ITER).t() - dist_t).abs().max())
    print(f"chunk method_boot={method_boot}: max |grouped - per trial| = {diff:.3e}", flush=True)
