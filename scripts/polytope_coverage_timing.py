#!/usr/bin/env python3
"""Timing of the polytope coverage study (quantpy_amd.tomography.polytopes.verification) per row of the reference's
figure: GHZ(1..5) at 1e4 shots, depolarizing(0.1, n = 1..3) at 1e4 shots, depolarizing(0.1, 1) at 1e2 ... 1e5 shots;
18 confidence levels.

Per row: the device sampler's time and the coverage kernels' time (HIP events around the launches of every chunk, the
arrays already on the device), the end-to-end wall time of test_qst / test_qpt with sampler='device', and the host
loop -- utils.count_delta per trial and level, one core -- on a bounded sample of the same counts (at most
--host-seconds of it per row), extrapolated to the row's trials.  Prints one JSON line.

    python scripts/polytope_coverage_timing.py --trials 10000
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quantpy_amd as qp  # noqa: E402
from quantpy_amd import _capi  # noqa: E402
from quantpy_amd.engine import any_engine  # noqa: E402
from quantpy_amd.tomography.polytopes import utils, verification  # noqa: E402

LEVELS = np.concatenate((np.arange(0.1, 0.9, 0.1), np.arange(0.9, 1, 0.01)))
ROWS = ([("state", n, 10**4) for n in range(1, 6)] + [("channel", n, 10**4) for n in range(1, 4)]
        + [("channel", 1, 10**k) for k in range(2, 6)])


def dptr(t):
    return ctypes.c_void_p(t.data_ptr())


def time_row(kind, n, shots, trials, host_seconds, seed):
    if kind == "state":
        obj = qp.qobj.GHZ(n)
        probas, n_meas, truth = verification.qst_setup(obj, shots)
        run = lambda t: verification.test_qst(obj, LEVELS, shots, t, sampler="device", seed=seed)  # noqa: E731
    else:
        obj = qp.channel.depolarizing(p=0.1, n_qubits=n)
        probas, n_meas, truth = verification.qpt_setup(obj, shots)
        run = lambda t: verification.test_qpt(obj, LEVELS, shots, t, sampler="device", seed=seed)  # noqa: E731
    R, K = probas.shape
    L = LEVELS.size
    eng = any_engine()
    run(min(trials, 64))  # warm-up: library load, buffers
    t0 = time.perf_counter()
    fractions = run(trials)
    end_to_end = time.perf_counter() - t0

    # the same chunks, launches timed with HIP events on the engine's stream
    eng._dev_call()
    dev = torch.device("cuda", eng.device)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d_n, d_p, d_shots, d_levels, d_truth = to(n_meas.astype(np.int64)), to(probas), to(n_meas), to(LEVELS), to(truth)
    d_cov = torch.zeros(L, dtype=torch.int64, device=dev)
    chunk = verification.chunk_trials(trials, R * K, L)
    sample_ms = kernel_ms = worst_launch_ms = 0.0
    first_chunk = None
    for start in range(0, trials, chunk):
        size = min(chunk, trials - start)
        counts = torch.empty((size, R, K), dtype=torch.int64, device=dev)
        eng.timer_begin()
        eng.device_multinomial(d_n, d_p, size * R, seed, first_row=start * R, out=counts)
        sample_ms += eng.timer_end()
        eng.timer_begin()
        eng._chk(eng.lib.qt_polytope_coverage(eng._h, dptr(counts), size, R, K, dptr(d_shots), dptr(d_levels), L,
                                              dptr(d_truth), int(kind == "state"), None, None, dptr(d_cov),
                                              _capi.QT_DEVICE_PTR))
        ms = eng.timer_end()
        kernel_ms += ms
        worst_launch_ms = max(worst_launch_ms, ms)
        if first_chunk is None:
            first_chunk = counts[: min(size, 64)].cpu().numpy()
    assert np.array_equal(d_cov.cpu().numpy() / trials, fractions)  # the same stream, the same chunks

    # host loop on a bounded sample of the same counts
    calls, t0 = 0, time.perf_counter()
    for table in first_chunk:
        freq = np.clip(table / n_meas[:, None], 1e-15, 1 - 1e-15)
        for cl in LEVELS:
            utils.count_delta(cl, freq, n_meas)
            calls += 1
        if time.perf_counter() - t0 > host_seconds:
            break
    host_per_call = (time.perf_counter() - t0) / calls
    evaluations = trials * L * 34 * R * K
    return {"kind": kind, "n_qubits": n, "shots": shots, "R": R, "K": K, "trials": trials, "chunk": chunk,
            "sample_ms": round(sample_ms, 3), "kernel_ms": round(kernel_ms, 3), "worst_launch_ms": round(worst_launch_ms, 3),
            "end_to_end_ms": round(end_to_end * 1e3, 3), "kernel_evaluations_per_s": round(evaluations / (kernel_ms * 1e-3), -6),
            "host_count_delta_ms": round(host_per_call * 1e3, 4), "host_calls_timed": calls,
            "host_extrapolated_s": round(host_per_call * trials * L, 1),
            "speedup_end_to_end": round(host_per_call * trials * L / end_to_end, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=10000)
    ap.add_argument("--host-seconds", type=float, default=2.0)
    ap.add_argument("--rows", type=int, nargs="*", default=list(range(len(ROWS))))
    ap.add_argument("--seed", type=int, default=20261016)
    args = ap.parse_args()
    rows = [time_row(*ROWS[i], args.trials, args.host_seconds, args.seed + i) for i in args.rows]
    print(json.dumps({"polytope_coverage_timing": rows, "levels": int(LEVELS.size),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
