"""Where the time of MomentInterval on a three-qubit process goes (ProcessTomograph, 'proj-set': 64 input states x 27
settings x 8 outcomes = 13 824 rows): design matrix (host einsum), left inverse (qt_left_inverse), and the moment call
(host copy of the 453 MB left inverse, W = P^T P, k_moment_cols + k_moment_finish) for 1 and 64 trials.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own times.  With --numpy it times the NumPy matrix form of the same
sums for one trial instead, on one host core (threadpoolctl)."""
import sys
import time

import numpy as np
from threadpoolctl import threadpool_info, threadpool_limits

sys.path.insert(0, ".")
import quantpy_amd as qp  # noqa: E402
from quantpy_amd.routines import _left_inv  # noqa: E402


def numpy_matrix_form(inv, freq, n_trials, k):
    f = freq.reshape(-1)
    m, s = f.size, f.size // k
    w = inv.T @ inv
    u = (w * f[:, None]).reshape(s, k, m).sum(1)
    q = (u * f[None, :]).reshape(s, s, k).sum(2)
    uuf, wwf, t_d = (u * u * f[None, :]).sum(), f @ ((w * w) @ f), np.diagonal(w) @ f
    q2, tr_q = (q * q).sum(), np.trace(q)
    first = (t_d - tr_q) / n_trials
    return first, ((tr_q - t_d) ** 2 + 2 * q2 - 4 * uuf + 2 * wwf) / n_trials**2 - first * first


np.random.seed(1)
tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
counts = tmg.experiment_batch(1000, "proj-set", repeats=64)
first = tmg.tomographs[0]
t0 = time.perf_counter()
povm_rows = np.asarray(first.povm_matrix).reshape(-1, first.povm_matrix.shape[-1])
states = np.asarray([rho.T.bloch for rho in tmg.input_basis.elements])
design = np.einsum("sd,pi->spdi", states, povm_rows).reshape(states.shape[0] * povm_rows.shape[0], -1)
t1 = time.perf_counter()
inv = np.asarray(_left_inv(design)) / 4**3
t2 = time.perf_counter()
print(f"design matrix {design.shape}: {1e3 * (t1 - t0):.1f} ms (host) | left inverse {inv.shape}: {1e3 * (t2 - t1):.1f} ms")
ns = np.tile(first.n_measurements, len(tmg.tomographs)).astype(np.float64)
c = counts.reshape(64, -1, counts.shape[-1])
eng = qp.get_engine(3)
if "--numpy" in sys.argv:
    p = np.ascontiguousarray(inv, dtype=np.float64)
    with threadpool_limits(limits=1):
        print("BLAS threads:", [(lib["internal_api"], lib["num_threads"]) for lib in threadpool_info()])
        t0 = time.perf_counter()
        m0, v0 = numpy_matrix_form(p, c[0] / ns[:, None], ns[0], c.shape[-1])
        t1 = time.perf_counter()
    m1, v1 = eng.moments(c[0], ns, inv)
    print(f"NumPy matrix form, one trial: {t1 - t0:.2f} s | mean {m0!r} vs {m1!r} | variance {v0!r} vs {v1!r}")
else:
    for batch in (1, 64, 1, 64):  # the first pair allocates W and the staging buffers
        t0 = time.perf_counter()
        mean, var = eng.moments(c[:batch], ns, inv)
        t1 = time.perf_counter()
        print(f"eng.moments, {batch} trial(s), host pointers: {1e3 * (t1 - t0):.1f} ms | mean[0] {mean[0]!r} variance[0] {var[0]!r}")
