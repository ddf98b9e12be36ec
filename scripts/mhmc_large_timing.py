"""Timing of MHMCStateInterval.setup() (reference interval.py:689-750, mhmc.py) at n = 4, 5 with n_points = 1000 and
burn_steps = 1000 ('proj-set', 1000 shots per setting, a full-rank state): 2000 chain steps.  Per n: the whole setup()
on the host clock (second call; the first one warms the library), the one qt_mhmc_state call between HIP events (the
kernel and the staging of its 2000 x 4^n proposal increments), and the oracle's NumPy chain (the reference's arithmetic)
on one host core over the first 200 (n = 4) / 40 (n = 5) steps, scaled to 2000.  --no-numpy skips the NumPy chain (for a rocprofv3
--kernel-trace --stats run, which reports k_mhmc_state_large's own time)."""
import sys
import time

import numpy as np
from threadpoolctl import threadpool_limits

sys.path.insert(0, ".")
sys.path.insert(0, "oracle")
import quantpy_amd as qp  # noqa: E402
import quantpy_oracle as qo  # noqa: E402

numpy_chain = "--no-numpy" not in sys.argv
numpy_steps = {4: 200, 5: 40}
n_points, burn = 1000, 1000
for n in (4, 5):
    d = 2**n
    rng = np.random.default_rng(n)
    g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
    rho = g @ g.conj().T
    rho /= np.trace(rho)
    np.random.seed(n)
    tmg = qp.StateTomograph(qp.Qobj(rho))
    tmg.experiment(1000)
    tmg.reconstructed_state = qp.Qobj(rho)
    qp.MHMCStateInterval(tmg, n_points=n_points, burn_steps=burn).setup()
    iv = qp.MHMCStateInterval(tmg, n_points=n_points, burn_steps=burn)
    t0 = time.perf_counter()
    iv.setup()
    t1 = time.perf_counter()
    eng = tmg._engine()
    T = n_points + burn
    x0, _ = eng.chol_param(rho)
    deltas = np.random.standard_normal((T, d * d))
    uniforms = np.random.rand(T)
    eng.mhmc_state(tmg.results, x0, deltas, uniforms, 0.01)
    eng.timer_begin()
    chain, acc = eng.mhmc_state(tmg.results, x0, deltas, uniforms, 0.01)
    call_ms = eng.timer_end()
    line = (f"n={n} ({T} steps): setup() {1e3 * (t1 - t0):8.2f} ms | qt_mhmc_state (HIP events) {call_ms:8.3f} ms"
            f" = {1e3 * call_ms / T:6.2f} us/step | acceptance {acc.mean():.3f}")
    if numpy_chain:
        k = numpy_steps[n]
        povm = qo.measurement_matrix("proj-set", n)
        with threadpool_limits(limits=1):
            t2 = time.perf_counter()
            ref, ref_acc = qo.mhmc_state_chain(tmg.results, povm, x0, deltas[:k], uniforms[:k], 0.01)
            t3 = time.perf_counter()
        assert np.abs(ref - chain[:k]).max() < 1e-12 and np.array_equal(ref_acc, acc[:k])
        per = (t3 - t2) / k
        line += f" | NumPy chain, one core: {1e6 * per:9.1f} us/step ({k} steps), {per * T:7.2f} s for {T} steps"
    print(line, flush=True)
