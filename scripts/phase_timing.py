"""Per-wave phase breakdown of the n = 3 kernels (bench workload) from in-kernel shader-clock stamps.
Needs the profile build:  python -c "from quantpy_amd.build import build_profile_library as b; b()"
and QTOMO_LIB=quantpy_amd/lib/libqtomo_prof.so in the environment."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import quantpy_amd as qp  # noqa: E402
from quantpy_amd.tomography.state import simulate_counts  # noqa: E402

n, d, B = 3, 8, 1000
rng = np.random.default_rng(1234)
g = rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d))
rho = g @ g.conj().T
rho /= np.trace(rho).real
povm = qp.generate_measurement_matrix("proj-set", n)
shots = np.ones(povm.shape[0]) * 100000
np.random.seed(7)
counts = np.stack([simulate_counts(povm, qp.Qobj(rho).bloch, shots) for _ in range(B)])
eng = qp.get_engine(n, device=0)
eng.set_povm(povm, shots)
cd_ = torch.from_numpy(counts).cuda()
out = torch.empty((B, d, d), dtype=torch.complex128, device="cuda")
ROWS = B + 8  # one per trial wavefront (whole workgroups); k_mle_fused_hw's twin wavefronts stamp the rows behind them
prof = torch.zeros((2 * ROWS, 32), dtype=torch.int64, device="cuda")
eng.lib.qt_debug_set_prof.argtypes = [ctypes.c_void_p]
assert eng.lib.qt_debug_set_prof(prof.data_ptr()) == 0
names = {0: "start", 1: "load_freq", 2: "lin_invert", 3: "cholesky #1", 4: "gauss-jordan inverse", 5: "squarings",
         6: "lift tail / jacobi", 7: "cholesky #2", 8: "make_feasible end", 9: "nll_grad end + gnorm", 10: "store",
         11: "(nll) entry", 12: "(nll) build L L^H", 13: "(nll) bloch_of", 14: "(nll) fwd stages 1..n-1",
         15: "(nll) stage n + log", 16: "(nll) backward stages", 17: "(nll) matrix_of", 18: "(nll) Gt L + tail", 19: "deferred value",
         25: "(nll) wait for helper", 31: "wait for the lifted matrix"}
# 9 closes the first evaluation and its gradient norm; 19 is stamped only by the waves that form the deferred value
# (a trial that iterates, a caller that asks for `fun`, a p outside the logarithm's regular range).  k_mle_fused_hw:
# a clipped trial's first wave stamps 31 when the lifted matrix has arrived (its wait starts at the verdict behind
# "cholesky #1") and 7 when its sweep for the twin is done; everything behind that is in the twin's row (HELPER below)
ORDER = [1, 2, 3, 31, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 25, 18, 9, 19, 10]
# A twin wavefront's stamps, in clocks since ITS TRIAL's start: slot 0 = its own start (behind the barrier of make_ctx),
# 1 = its load_freq done, 2 = its lin_invert done: the inverse starts (the matrix is in its registers), 4 = inverse done,
# 26 .. 30 = squarings 1 .. 5, 5 = squarings done, 6 = lift over (tail done, refused or called off), 7 = verdict "go"
# seen, 8 = lifted matrix published: from here the twin owns the trial and stamps the trial's slots (17 front of
# nll_grad, 25 x received from the other wave, 18, 9, 10) in its own row.  The second sweep's end is slot 7 of the FIRST
# wave's row (sweep_for).
HELPER = [(0, "twin starts"), (1, "own load_freq done"), (2, "own lin_invert done"), (4, "inverse done"), (26, "squaring 1"), (27, "squaring 2"), (28, "squaring 3"),
          (29, "squaring 4"), (30, "squaring 5"), (5, "squarings done"), (6, "lift over"), (7, "verdict go seen"),
          (8, "matrix published, owns the trial"), (17, "front of nll_grad done"), (25, "x received"), (18, "nll_grad done"),
          (9, "gnorm"), (10, "store")]


def mle(helper):
    eng.set_option(qp._capi.QT_OPT_MLE_HELPER_WAVE, helper)
    eng.mle_dev(cd_, out)


for name, fn in (("k_lin_batch", lambda: eng.lin_dev(cd_, out, physical=True)), ("k_mle_fused", lambda: mle(0)),
                 ("k_mle_fused_hw", lambda: mle(1))):
    for _ in range(3):
        fn()
    eng.sync()
    prof.zero_()
    eng.timer_begin()
    fn()
    ms = eng.timer_end()
    both = prof.cpu().numpy()
    # the helpers' rows start behind the rows of the whole grid: B rounded up to whole workgroups of four trials
    p, ph = both[:B], both[(B + 3) // 4 * 4:][:B]
    span = (p.max(1) - p[:, 0])
    nonpd = p[:, 6] > 0
    print(f"== {name}: {ms * 1e3:.1f} us for {B} trials; slowest wave {span.max()} clk, {nonpd.sum()} non-PD trials")
    if nonpd.any():
        src = ph if ph[nonpd, 20].any() else p  # k_mle_fused_hw: the squarings run in the helper wavefronts
        ks = src[nonpd, 20]
        sq = src[nonpd, 5] - src[nonpd, 4]
        for k in np.unique(ks):
            print(f"  squarings = {k}: {np.sum(ks == k)} waves, phase mean {sq[ks == k].mean():.0f} max {sq[ks == k].max()} clk")
    for label, sel in (("PD trials", ~nonpd), ("non-PD trials", nonpd)):
        if not sel.any():
            continue
        q = p[sel]
        print(f"  {label}: mean total {np.mean(q.max(1) - q[:, 0]):.0f} clk")
        prev = q[:, 0]
        for s in ORDER:
            cur = q[:, s]
            have = cur > 0
            if not have.any():
                continue
            dt = (cur - prev)[have]
            print(f"    {names[s]:24s} mean {dt.mean():8.0f}  max {dt.max():8.0f} clk  ({have.sum()} waves)")
            prev = np.where(have, cur, prev)
    if ph.any():
        for label, sel in (("PD trials", ~nonpd), ("non-PD trials", nonpd)):
            print(f"  twin wavefronts of the {label} (clocks since the trial's start):")
            for slot, what in HELPER:
                have = sel & (ph[:, slot] > 0)
                if have.any():
                    at = (ph[:, slot] - p[:, 0])[have]
                    print(f"    {what:24s} mean {at.mean():8.0f}  max {at.max():8.0f} clk  ({have.sum()} waves)")
        # the trial's stamps on the same scale, for the clipped trials: verdict, matrix received, sweep for the twin done
        for slot, what in ((2, "lin_invert done"), (3, "verdict (cholesky #1 done)"), (31, "lifted matrix received"),
                           (7, "sweep for the twin done")):
            have = nonpd & (p[:, slot] > 0)
            if have.any():
                at = (p[:, slot] - p[:, 0])[have]
                print(f"  trial wavefront, non-PD: {what:28s} mean {at.mean():8.0f}  max {at.max():8.0f} clk")
        owns = ph[:, 10] > 0
        print(f"  {owns.sum()} twins own their trial's outputs; slowest of them {(ph[owns].max(1) - p[owns, 0]).max() if owns.any() else 0} clk")
