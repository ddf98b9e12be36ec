"""Timing of the five-qubit polytope programs (A 7776 x 1023) on qt_lp_ineq_xl_batch: 'proj-set', 1000 shots, a
depolarised GHZ state against GHZ, the right-hand sides of StateFidelityIntervalXL with n_points = 1000.
 (a) 4 programs (the two ends of the widening range, both signs of c), one per workgroup: HIP events, one warm-up call
     and REPEATS timed ones -> kernel time per program and per iteration;
 (b) one full launch: kLaunchProgramsXL = 256 programs on 256 workgroups, the same way (one timed run);
 (c) one setup() with n_points = 1000 (2000 programs, 8 launches) on the host clock, after (a) and (b) as warm-up;
 (d) with --highs: HiGHS (scipy.optimize.linprog) on one host core for one of the programs of (a) (about 40 s).
--quick runs (a) only."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import quantpy_amd as qp  # noqa: E402
from quantpy_amd.tomography.polytopes import StateFidelityIntervalXL  # noqa: E402
from quantpy_amd.tomography.polytopes.fidelity import kLaunchProgramsXL  # noqa: E402

REPEATS = 3


def spread(ms):
    return f"min {min(ms):9.2f} / median {float(np.median(ms)):9.2f} / max {max(ms):9.2f} ms"


np.random.seed(1)
ghz = qp.qobj.GHZ(5)
tmg = qp.StateTomograph(qp.channel.depolarizing(0.1, 5).transform(ghz))
tmg.experiment(1000, "proj-set")
interval = StateFidelityIntervalXL(tmg, n_points=1000, target_state=ghz)
A, b, c, _, _ = interval.programs()
C = np.stack([c, -c])
eng = qp.get_engine(5)

ends = b[[0, -1]]
eng.lp_ineq_xl_batch(A, C, ends)
ms = []
for _ in range(REPEATS):
    eng.timer_begin()
    obj, status, iters = eng.lp_ineq_xl_batch(A, C, ends)
    ms.append(eng.timer_end())
med = float(np.median(ms))
print(f"(a) A {A.shape}: qt_lp_ineq_xl_batch, 4 LPs on 4 workgroups, HIP events: {spread(ms)} | iterations "
      f"{iters.ravel().tolist()} | statuses {status.ravel().tolist()} | {med / iters.max():.2f} ms per iteration of the "
      f"longest program", flush=True)
if "--highs" in sys.argv:
    from scipy.optimize import linprog

    t0 = time.perf_counter()
    res = linprog(C[0], A_ub=A, b_ub=ends[0], bounds=[(None, None)] * A.shape[1], method="highs")
    print(f"(d) HiGHS, the first of those programs, one host core: {time.perf_counter() - t0:.1f} s, status {res.status}, "
          f"relative difference {abs(res.fun - obj[0, 0]) / max(1.0, abs(res.fun)):.1e}", flush=True)
if "--quick" not in sys.argv:
    rows = np.linspace(0, len(b) - 1, kLaunchProgramsXL // 2).round().astype(int)
    eng.timer_begin()
    obj, status, iters = eng.lp_ineq_xl_batch(A, C, b[rows])
    one = eng.timer_end()
    print(f"(b) one launch of {status.size} LPs on {status.size} workgroups, HIP events: {one:.2f} ms | iterations "
          f"{iters.min()}-{iters.max()} (mean {iters.mean():.1f}) | statuses {np.bincount(status.ravel()).tolist()} | "
          f"{one / iters.max():.2f} ms per iteration of the longest program", flush=True)
    t0 = time.perf_counter()
    interval.setup()
    wall = time.perf_counter() - t0
    it = interval.lp_iters
    print(f"(c) StateFidelityIntervalXL.setup(), n_points = 1000: {it.size} LPs in {-(-it.size // kLaunchProgramsXL)} "
          f"launches, host clock {wall:.2f} s | iterations {it.min()}-{it.max()} (mean {it.mean():.1f}) | statuses "
          f"{np.bincount(interval.lp_status.ravel()).tolist()}", flush=True)
