"""Timing of the polytope fidelity bounds (quantpy_amd.tomography.polytopes.fidelity), 'proj-set', 1000 shots:
 (a) ProcessFidelityInterval at n = 2 ('sic' inputs), n_points = 1000: 2000 LPs with A 576 x 240;
 (b) StateFidelityInterval at n = 4, n_points = 1000: 2000 LPs with A 1296 x 255;
 (c) the figure-2a study at n = 1: fidelity_qpt with 100 trials x 30 levels at 1e3, 1e4, 1e5 shots (18 000 LPs, N = 12);
 (d) the whole setup() of (a) and (b) on the host clock.
For (a), (b): the one qt_lp_ineq_large_batch launch between HIP events, one warm-up and REPEATS timed runs (min / median
/ max).  For (c): the wall clock of each call (sampling, bisection, right-hand sides, LPs), the same way, and the NumPy
assembly of its right-hand sides alone.  HiGHS (scipy.optimize.linprog) on one host core for SAMPLE programs of each.
--no-highs skips the HiGHS loops (for a rocprofv3 --kernel-trace --stats run, which reports the kernels' own time)."""
import sys
import time

import numpy as np
from scipy.optimize import linprog

sys.path.insert(0, ".")
import quantpy_amd as qp  # noqa: E402
from quantpy_amd.tomography.polytopes import ProcessFidelityInterval, StateFidelityInterval, fidelity_qpt  # noqa: E402

REPEATS, SAMPLE = 5, 8
highs = "--no-highs" not in sys.argv


def spread(ms):
    return f"min {min(ms):9.2f} / median {float(np.median(ms)):9.2f} / max {max(ms):9.2f} ms"


def highs_sample(A, C, b, obj, status):
    rows = np.linspace(0, b.shape[0] - 1, SAMPLE // 2).round().astype(int)
    t0 = time.perf_counter()
    worst = 0.0
    for r in rows:
        for o in range(2):
            res = linprog(C[o], A_ub=A, b_ub=b[r], bounds=[(None, None)] * A.shape[1], method="highs")
            if res.status == 0 and status[r, o] == 0:
                worst = max(worst, abs(res.fun - obj[r, o]) / max(1.0, abs(res.fun)))
    per = (time.perf_counter() - t0) / (2 * len(rows))
    return f"HiGHS {1e3 * per:8.1f} ms per LP ({2 * len(rows)} of them), worst rel. difference {worst:.1e}"


np.random.seed(1)
cases = []
tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 2), input_states="sic")
tmg.experiment(1000, "proj-set")
cases.append(("(a) process n=2", 2, lambda: ProcessFidelityInterval(tmg, n_points=1000, target_channel=qp.channel.depolarizing(0, 2))))
ghz = qp.qobj.GHZ(4)
tms = qp.StateTomograph(qp.channel.depolarizing(0.1, 4).transform(ghz))
tms.experiment(1000, "proj-set")
cases.append(("(b) state n=4  ", 4, lambda: StateFidelityInterval(tms, n_points=1000, target_state=ghz)))
for name, n, make in cases:
    make().setup()
    host = []
    for _ in range(3):
        iv = make()
        t0 = time.perf_counter()
        iv.setup()
        host.append(1e3 * (time.perf_counter() - t0))
    A, b, c, _, _ = iv.programs()
    C = np.stack([c, -c])
    eng = qp.get_engine(n)
    eng.lp_ineq_large_batch(A, C, b)
    ms = []
    for _ in range(REPEATS):
        eng.timer_begin()
        obj, status, iters = eng.lp_ineq_large_batch(A, C, b)
        ms.append(eng.timer_end())
    line = (f"{name} A {A.shape}: qt_lp_ineq_large_batch, {status.size} LPs, HIP events: {spread(ms)} | iterations "
            f"{iters.min()}-{iters.max()} (mean {iters.mean():.1f}) | statuses {np.bincount(status.ravel()).tolist()}"
            f" | (d) setup() host clock: {spread(host)}")
    if highs:
        line += " | " + highs_sample(A, C, b, obj, status)
    print(line, flush=True)

# (c) the study of Fig. 2a at n = 1
channel, target = qp.channel.depolarizing(0.1, 1), qp.channel.depolarizing(0, 1)
levels = 1 - np.array(list(np.logspace(-5, -0.2, 20)) + list(np.linspace(0.65, 0.99, 10)))
for shots in (1000, 10000, 100000):
    np.random.seed(2)
    fidelity_qpt(channel, target, levels, n_measurements=shots, n_trials=100)
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        f_min, f_max, table = fidelity_qpt(channel, target, levels, n_measurements=shots, n_trials=100, return_table=True)
        ms.append(1e3 * (time.perf_counter() - t0))
    it = table["lp_iters"]
    print(f"(c) fidelity_qpt n=1, {shots} shots, 100 trials x 30 levels = {it.size} LPs, wall clock: {spread(ms)} | "
          f"iterations {it.min()}-{it.max()} (mean {it.mean():.1f}) | statuses {np.bincount(table['lp_status'].ravel()).tolist()}"
          f" | NaN bounds {int(np.isnan(f_min).sum())}", flush=True)
# the right-hand sides of one such call, assembled with NumPy as _study does: 3000 x 24 doubles
freq = np.random.rand(100, 1, 24)
dl = np.random.rand(100, 30)
ms = []
for _ in range(20):
    t0 = time.perf_counter()
    rhs = (freq + dl[:, :, None] - 0.5).reshape(3000, 24)
    ms.append(1e3 * (time.perf_counter() - t0))
print(f"    right-hand sides of one call (NumPy broadcast, {rhs.shape}): {spread(ms)}", flush=True)
