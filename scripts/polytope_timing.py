"""Timing of PolytopeStateInterval.setup() (reference interval.py:268-335: 2 * n_points LPs) at n = 1, 2, 3 with
n_points = 1000, 'proj-set', 1000 shots per setting.  Per n: the whole setup() on the host clock (second call; the
first one warms the library), the one qt_lp_ineq_batch launch between HIP events, and the same 2000 LPs through HiGHS
(scipy.optimize.linprog) on one host core.  --no-highs skips the HiGHS loop (for a rocprofv3 --kernel-trace --stats
run, which reports k_lp_ineq's own time)."""
import sys
import time

import numpy as np
from scipy.optimize import linprog

sys.path.insert(0, ".")
import quantpy_amd as qp  # noqa: E402

highs = "--no-highs" not in sys.argv
np.random.seed(1)
for n in (1, 2, 3):
    d = 2**n
    rng = np.random.default_rng(n)
    g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = g @ g.conj().T
    tmg = qp.StateTomograph(qp.Qobj(rho / np.trace(rho)))
    tmg.experiment(1000)
    qp.PolytopeStateInterval(tmg, n_points=1000).setup()
    iv = qp.PolytopeStateInterval(tmg, n_points=1000)
    t0 = time.perf_counter()
    iv.setup()
    t1 = time.perf_counter()
    A, b, c, _, _ = iv.programs()
    eng = qp.get_engine(n)
    C = np.stack([c, -c])
    eng.lp_ineq_batch(A, C, b)
    eng.timer_begin()
    obj, status, iters = eng.lp_ineq_batch(A, C, b)
    kernel_ms = eng.timer_end()
    line = (f"n={n} A {A.shape}: setup() {1e3 * (t1 - t0):8.2f} ms | qt_lp_ineq_batch (2000 LPs, HIP events) {kernel_ms:7.3f} ms"
            f" | iterations {iters.min()}-{iters.max()} (mean {iters.mean():.1f}) | statuses {np.bincount(status.ravel()).tolist()}")
    if highs:
        t2 = time.perf_counter()
        worst = 0.0
        for r in range(b.shape[0]):
            for o in range(2):
                res = linprog(C[o], A_ub=A, b_ub=b[r], bounds=[(None, None)] * A.shape[1], method="highs")
                if res.status == 0 and status[r, o] == 0:
                    worst = max(worst, abs(res.fun - obj[r, o]) / max(1.0, abs(res.fun)))
        t3 = time.perf_counter()
        line += f" | HiGHS, same LPs: {1e3 * (t3 - t2):8.1f} ms, worst rel. difference {worst:.1e}"
    print(line, flush=True)
