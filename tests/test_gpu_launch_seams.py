"""GPU: the seams of the host code that plans a launch (csrc/qtomo.hip) -- where a batch is cut, how the per-trial pointers
are offset behind the cut, and which kernel variant runs.  Every size here is the smallest that crosses its seam.

The pattern: the batch in ONE call past the seam ("whole") against the same trials in calls that each stay inside one piece
("pieces"), bit for bit in every output, and against an independent reference (the CPU oracle, NumPy) on trials on both
sides of the seam at the tolerance the neighbouring test of that kernel uses.  Every trial of a batch is drawn on its own,
so an offset that lands on another trial changes the numbers."""
import numpy as np
import pytest
from conftest import load_golden
from test_gpu_moments_large import check as check_moments
from test_gpu_moments_large import large_case, make_inputs

pytestmark = pytest.mark.gpu

KLDS = 160 * 1024  # kLdsLimit: the LDS of a CU, all of which one workgroup may use


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def ginibre(rng, d, rank=None):
    r = d if rank is None else rank
    g = rng.standard_normal((d, r)) + 1j * rng.standard_normal((d, r))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


_POVM = {}


def proj_set(qp, n):
    """'proj-set' as the engine takes it and as a dense (S, K, 4^n) array."""
    if n not in _POVM:
        a = qp.generate_measurement_matrix("proj-set", n)
        _POVM[n] = (a, np.asarray(a))
    return _POVM[n]


def draw_trials(oracle, ad, shots, batch, seed):
    """`batch` trials, each its own multinomial draw per setting: Born probabilities of six random states, alternating full
    rank and rank 2, cycled over the batch."""
    d = int(round(ad.shape[-1] ** 0.5))
    rng = np.random.default_rng(seed)
    states = [ginibre(rng, d, None if i % 2 == 0 else 2) for i in range(6)]
    p = np.stack([oracle.born_probs(ad, oracle.bloch_from_matrix(s)) for s in states])
    p /= p.sum(-1, keepdims=True)
    return np.stack([rng.multinomial(shots, p[b % 6]) for b in range(batch)]).astype(np.int64)


def lds_cap(n):
    """The largest max_iter whose BFGS launch fits KLDS with 'proj-set' (M = 6^n rows, one-qubit table of R1 = 6 rows),
    restated from Small<3>::lds_bytes and Large<NQ>::lds_bytes, in doubles.
    n = 3 (split pair, 4 trials per workgroup): tables 976 / 2 + 216 + 48 = 752 once, and per trial the scratch
    362 + 3 * 216 = 1010, the parked line-search state 32 and 2 per iteration; the compiled k_mle_bfgs<3, .> holds 256 B
    = 32 doubles of LDS of its own (profiles/bfgs_loop_resources.txt; the library asks hipFuncGetAttributes), which the
    dynamic part cannot have: 32 + 752 + 4 (1042 + 2 max_iter) <= 20480.
    n = 4, 5 (one trial per workgroup, kernels without LDS of their own): oTab = MAT + D + d + 32 + 32, + 8 R1 + max(M, MAT)
    + max(4 M / R1, MAT), and 2 per iteration: 3088 + 2 max_iter (n = 4), 16240 + 2 max_iter (n = 5) <= 20480."""
    m, r1, d, dd = 6**n, 6, 2**n, 4**n
    if n == 3:
        tables = (456 + 304 + m + 1) // 2 * 2 // 2 + m + 8 * r1
        trial = 362 + 3 * m + 32
        return (KLDS // 8 - 32 - tables - 4 * trial) // 8
    mat = 2 * (d + 1) * d
    base = mat + dd + d + 32 + 32 + 8 * r1 + max(m, mat) + max(4 * m // r1, mat)
    return (KLDS // 8 - base) // 2


# n, max_iter (the real cap: the documented ceilings are 2000 at n = 3 and 4096 at n = 4, 5), shots per setting
CAPS = [(3, 1941, 1000), (4, 4096, 300), (5, 2120, 2000)]


def test_caps_follow_from_the_lds_layout():
    assert [min(lds_cap(n), 2000 if n == 3 else 4096) for n, _, _ in CAPS] == [c for _, c, _ in CAPS]


def _mle_outputs(eng, counts, max_iter):
    rho, info = eng.mle(counts, max_iter=max_iter, return_info=True)
    return dict(rho=rho, **info)


def _grouped_mle(eng, counts_d, table_d, max_iter):
    """mle_dist_dev on an engine with a stream of its own: every output as a NumPy array."""
    import torch

    b, d = counts_d.shape[0], table_d.shape[-1]
    out = dict(dist=torch.empty(b, dtype=torch.float64, device="cuda"),
               rho=torch.empty((b, d, d), dtype=torch.complex128, device="cuda"),
               nit=torch.empty(b, dtype=torch.int32, device="cuda"), nfev=torch.empty(b, dtype=torch.int32, device="cuda"),
               fun=torch.empty(b, dtype=torch.float64, device="cuda"), status=torch.empty(b, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    eng.mle_dist_dev(counts_d, table_d, out["dist"], max_iter=max_iter, rho=out["rho"], nit=out["nit"], nfev=out["nfev"],
                     fun=out["fun"], status=out["status"])
    eng.sync()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("n,max_iter,shots", CAPS)
def test_bfgs_history_chunks(qp, oracle, n, max_iter, shots):
    """mle_batch_impl runs the BFGS kernel of the split pair in chunks of at most 4 GiB of history (max_iter x 2 x 4^n doubles
    per trial), MleArrays::at(b0) offsetting eleven per-trial arrays and rotating the centre table by (g0 + b0) % G:
    chunk = floor(2^32 / (max_iter 2 4^n 8)) = 2160 trials at n = 3 with max_iter = 1941, 256 at n = 4 with 4096, 123 at
    n = 5 with 2120 (the caps of test_iteration_caps), and B = chunk + 3 puts three trials behind the seam.  At n = 3 every
    call takes the split pair (max_iter > 256).  Whole = pieces [0:chunk], [chunk:B] in every output; the oracle's BFGS on
    the trials around the seam (same nit, infidelity < 1e-6, as test_mle_vs_bfgs_restatement); and the grouped distance
    with seven centres (7 divides no chunk) across the seam, the second piece with the table rolled by chunk % 7.
    The engine is private and closed at the end: the 4 GiB of history must not stay with a cached engine."""
    import torch

    d = 2**n
    chunk = 2**32 // (max_iter * 2 * 4**n * 8)
    batch = chunk + 3
    assert chunk % 7 != 0
    a, ad = proj_set(qp, n)
    counts = draw_trials(oracle, ad, shots, batch, 1000 + n)
    rng = np.random.default_rng(2000 + n)
    centres = np.stack([ginibre(rng, d) for _ in range(7)])
    seam = [0, chunk - 1, chunk, batch - 1] if n < 5 else [chunk - 1, chunk]
    eng = qp.Engine(n, stream="own")
    try:
        eng.set_povm(a, counts[0].sum(-1))
        whole = _mle_outputs(eng, counts, max_iter)
        print("nit: min", whole["nit"].min(), "max", whole["nit"].max(), "behind the seam", whole["nit"][chunk:])
        assert whole["nit"].min() >= 1  # the history is written on both sides of the seam
        pieces = [_mle_outputs(eng, counts[lo:hi], max_iter) for lo, hi in ((0, chunk), (chunk, batch))]
        for k in whole:
            joined = np.concatenate([p[k] for p in pieces])
            differ = np.flatnonzero((whole[k] != joined).reshape(batch, -1).any(1))
            assert differ.size == 0, (k, "trials that differ from their piece:", differ[:8], "of", differ.size)
        for b in seam:
            ref, ri = oracle.mle_estimate(counts[b], ad, max_iter=max_iter, return_info=True, solver="port")
            print("trial", b, "nit", whole["nit"][b], ri["nit"], "infidelity", abs(oracle.infidelity(ref, whole["rho"][b])))
            assert whole["status"][b] == 0 and ri["status"] == 0
            assert whole["nit"][b] == ri["nit"], (b, whole["nit"][b], ri["nit"])
            assert abs(oracle.infidelity(ref, whole["rho"][b])) < 1e-6
        counts_d = torch.from_numpy(counts).cuda()
        table = torch.from_numpy(centres).cuda()
        rolled = torch.from_numpy(np.ascontiguousarray(np.roll(centres, -(chunk % 7), axis=0))).cuda()
        g_whole = _grouped_mle(eng, counts_d, table, max_iter)
        g_pieces = [_grouped_mle(eng, counts_d[:chunk].contiguous(), table, max_iter),
                    _grouped_mle(eng, counts_d[chunk:].contiguous(), rolled, max_iter)]
        for k in g_whole:
            joined = np.concatenate([p[k] for p in g_pieces])
            differ = np.flatnonzero((g_whole[k] != joined).reshape(batch, -1).any(1))
            assert differ.size == 0, ("grouped", k, "trials that differ from their piece:", differ[:8], "of", differ.size)
        assert np.array_equal(g_whole["rho"], whole["rho"])
        for b in [0, chunk - 1, chunk, batch - 1]:
            want = oracle.hs_dst(whole["rho"][b], centres[b % 7])
            assert abs(g_whole["dist"][b] - want) < 1e-13, (b, g_whole["dist"][b], want)
        del counts_d, table, rolled
    finally:
        eng.close()
        torch.cuda.empty_cache()


@pytest.mark.parametrize("n,cap,shots", CAPS)
def test_iteration_caps(qp, oracle, n, cap, shots):
    """The largest max_iter that runs, and the refusal one above it.  The two-loop scalars of every iteration share a CU's
    LDS with the POVM's scratch (lds_cap above): with 'proj-set' that allows 1941 iterations at n = 3, below the ceiling of
    2000; 8696 at n = 4, so the ceiling of 4096 holds; 2120 at n = 5, below the ceiling of 4096.  At the cap: status 0, and
    nit and rho as with max_iter = 300 (infidelity < 1e-6).  At cap + 1: QT_ERR_UNSUPPORTED from mle_batch_impl, the message
    naming the cap, before anything is launched -- the same engine then reproduces 'lin' and the earlier 'mle' bit for
    bit.
    Observed on an MI355X: 1941 / 4096 / 2120 ran (nit 2, 11, 4 / 5, 11, 4 / 1, 6, 1), rho bitwise equal to
    max_iter = 300; 1942 / 4097 / 2121 were refused with that code.  Before the cap was worked out, n = 3 launched its start
    kernel and then failed from 1942 on with QT_ERR_HIP (hipFuncSetAttribute(163840 B): invalid argument -- the 256 B the
    kernel holds by itself were not counted), leaving an error that the next set_povm of ANY engine reported as its own;
    n = 5, as the code read, was refused from 2121 on by launch()'s LDS check only after the start kernel had run."""
    from quantpy_amd import _capi

    a, ad = proj_set(qp, n)
    counts = draw_trials(oracle, ad, shots, 3, 3000 + n)
    eng = qp.get_engine(n)
    eng.set_povm(a, counts[0].sum(-1))
    lin = eng.lin(counts)
    short = _mle_outputs(eng, counts, 300)
    at_cap = _mle_outputs(eng, counts, cap)
    print("n", n, "cap", cap, "nit", at_cap["nit"], short["nit"], "bitwise", np.array_equal(at_cap["rho"], short["rho"]))
    assert np.all(at_cap["status"] == 0) and np.all(short["status"] == 0)
    assert np.array_equal(at_cap["nit"], short["nit"]) and np.all(at_cap["nit"] >= 1)
    for r0, r1 in zip(short["rho"], at_cap["rho"]):
        assert abs(oracle.infidelity(r0, r1)) < 1e-6
    with pytest.raises(qp.EngineError) as ei:
        eng.mle(counts, max_iter=cap + 1)
    print(ei.value)
    assert ei.value.code == _capi.QT_ERR_UNSUPPORTED
    assert str(cap) in str(ei.value) and "max_iter" in str(ei.value)
    assert np.array_equal(eng.lin(counts), lin)
    again = _mle_outputs(eng, counts, 300)
    for k in short:
        assert np.array_equal(again[k], short[k]), k


def test_n5_count_cache_on_and_off_in_the_bfgs_kernel(qp, oracle):
    """large_plan<5> puts a 32-bit R-order copy of the trial's counts (4 M + 8 B) behind everything else when it fits:
    (16240 + 2 max_iter) 8 + 31112 <= 163840, i.e. max_iter <= 175 in k_mle_large_bfgs<5> with 'proj-set'.  175 has the cache
    on, 176 reads the counts through pr.rmap (Large::freq).  The cache holds the same integers and no sum changes its order:
    nit, nfev, status and the bits of rho are equal.
    Observed on an MI355X: equal bit for bit (rho and fun), nit = 1, 7, 1."""
    a, ad = proj_set(qp, 5)
    counts = draw_trials(oracle, ad, 2000, 3, 4005)
    eng = qp.get_engine(5)
    eng.set_povm(a, counts[0].sum(-1))
    on = _mle_outputs(eng, counts, 175)
    off = _mle_outputs(eng, counts, 176)
    print("nit", on["nit"], off["nit"], "rho bitwise", np.array_equal(on["rho"], off["rho"]), "max |diff|",
          np.abs(on["rho"] - off["rho"]).max())
    assert np.all(on["nit"] >= 1) and np.all(on["status"] == 0)
    for k in ("nit", "nfev", "status"):
        assert np.array_equal(on[k], off[k]), k
    assert np.array_equal(on["rho"], off["rho"])
    assert np.array_equal(on["fun"], off["fun"])


def test_n5_registered_shots_beyond_32_bits(qp, oracle):
    """With 2^33 registered shots per setting no kernel at n = 5 takes the count cache (ns_max >= 2^32 in large_plan<5>):
    'lin', the NLL and 'mle' read 64-bit counts through pr.rmap.  The counts are those of a 2^20-shot draw times 2^13, so
    the frequencies are the same numbers and the totals exact: each result within 1e-12 of the 2^20 registration (cache on),
    and each against the oracle at the tolerances of test_lin_and_nll_golden and test_mle_vs_bfgs_restatement."""
    a, ad = proj_set(qp, 5)
    c20 = draw_trials(oracle, ad, 2**20, 3, 4105)
    c33 = c20 * 2**13
    assert c33.sum(-1).min() == 2**33 == c33.sum(-1).max()
    eng = qp.get_engine(5)
    got = {}
    for key, c in (("2^20", c20), ("2^33", c33)):
        eng.set_povm(a, c[0].sum(-1).astype(np.float64))
        lin = eng.lin(c)
        x, st = eng.chol_param(lin)
        assert np.all(st == 0)
        got[key] = dict(lin=lin, x=x, nll=eng.nll(x, c), **_mle_outputs(eng, c, 100))
    small, big = got["2^20"], got["2^33"]
    assert np.abs(big["lin"] - small["lin"]).max() < 1e-12
    assert np.abs(big["nll"][0] - small["nll"][0]).max() < 1e-12
    assert np.abs(big["nll"][1] - small["nll"][1]).max() < 1e-12 * max(1.0, np.abs(small["nll"][1]).max())
    assert np.array_equal(big["nit"], small["nit"]) and np.array_equal(big["status"], small["status"])
    assert np.abs(big["rho"] - small["rho"]).max() < 1e-12
    for b in range(3):
        want = oracle.lin_estimate(c33[b], ad)
        assert np.abs(big["lin"][b] - want).max() < 1e-11 and abs(oracle.infidelity(want, big["lin"][b])) < 1e-10
        fo, go = oracle.NllProblem(c33[b], ad).nll_and_grad(big["x"][b])
        assert abs(big["nll"][0][b] - fo) < 1e-11 and np.abs(big["nll"][1][b] - go).max() < 1e-9
        ref, ri = oracle.mle_estimate(c33[b], ad, return_info=True, solver="port")
        assert big["status"][b] == 0 and ri["status"] == 0
        assert big["nit"][b] == ri["nit"], (b, big["nit"][b], ri["nit"])
        assert abs(oracle.infidelity(ref, big["rho"][b])) < 1e-6


def test_n5_cached_count_of_33_bits_marks_its_trial(qp, oracle):
    """A cached trial (1000 registered shots, QT_OPT_SHOTS_CHECK = 0 so that only the width of a count can mark it) whose
    largest count is 2^32 - 1 -- |00000> measured with 2^32 - 1 shots per setting: the setting Z...Z puts all of them on one
    outcome -- passes with status 0 and the oracle's 'lin' (1e-10).  With that count at 2^32 the 32-bit copy would hold 0:
    Large::make_ctx's `wide` flag marks the trial TRIAL_SHOTS instead, and its two neighbours keep their bits."""
    import torch

    from quantpy_amd import _capi

    a, ad = proj_set(qp, 5)
    rng = np.random.default_rng(4205)
    zero = np.zeros((32, 32), dtype=np.complex128)
    zero[0, 0] = 1.0
    p = oracle.born_probs(ad, oracle.bloch_from_matrix(zero))
    top = 2**32 - 1
    wide = rng.multinomial(top, p / p.sum(-1, keepdims=True)).astype(np.int64)
    s_top, k_top = np.unravel_index(np.argmax(wide), wide.shape)
    assert wide[s_top, k_top] == top and (wide == top).sum() == 1 and np.all(wide.sum(-1) == top)
    near = draw_trials(oracle, ad, 1000, 2, 4206)
    batch = np.stack([near[0], wide, near[1]])
    eng = qp.get_engine(5)
    eng.set_povm(a, np.full(ad.shape[0], 1000.0))

    def lin(counts):
        cd = torch.from_numpy(counts).cuda()
        rho = torch.zeros((3, 32, 32), dtype=torch.complex128, device="cuda")
        st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        eng.lin_dev(cd, rho, status=st)
        return rho.cpu().numpy(), st.cpu().numpy()

    eng.set_option(_capi.QT_OPT_SHOTS_CHECK, 0)
    try:
        rho, st = lin(batch)
        assert st.tolist() == [0, 0, 0]
        err = np.abs(rho[1] - oracle.lin_estimate(wide, ad)).max()
        print("largest count 2^32 - 1: |rho - oracle| =", err)
        assert err < 1e-10
        batch[1, s_top, k_top] = 2**32
        rho2, st2 = lin(batch)
        assert st2.tolist() == [0, _capi.TRIAL_SHOTS, 0]
        assert np.array_equal(rho2[[0, 2]], rho[[0, 2]])
    finally:
        eng.set_option(_capi.QT_OPT_SHOTS_CHECK, 1)
    assert np.array_equal(eng.lin(near), rho[[0, 2]])


@pytest.mark.parametrize("n,batch,shots", [(4, 7, 300), (5, 5, 2000)])
def test_grouped_distances_at_n4_and_n5(qp, oracle, n, batch, shots):
    """qt_lin_dist_group_batch and qt_mle_dist_group_batch at n = 4, 5: k_lin_large and k_mle_large_* read
    o.centre_of(b, 2 D), trial b against centre b % 3.  rho equals the ungrouped entry's bit for bit, and dist[b] =
    hs_dst(rho[b], centre[b % 3]) within the 1e-13 of test_fused_distance_equals_two_pass."""
    import torch

    d = 2**n
    a, ad = proj_set(qp, n)
    counts = draw_trials(oracle, ad, shots, batch, 5000 + n)
    rng = np.random.default_rng(5100 + n)
    centres = np.stack([ginibre(rng, d) for _ in range(3)])
    eng = qp.get_engine(n)
    eng.set_povm(a, counts[0].sum(-1))
    cd = torch.from_numpy(counts).cuda()
    table = torch.from_numpy(centres).cuda()

    def outputs():
        return (torch.full((batch,), -1.0, dtype=torch.float64, device="cuda"),
                torch.zeros((batch, d, d), dtype=torch.complex128, device="cuda"),
                torch.full((batch,), -1, dtype=torch.int32, device="cuda"))

    def check(dist, rho, st, plain):
        dist, rho = dist.cpu().numpy(), rho.cpu().numpy()
        assert st.cpu().numpy().tolist() == [0] * batch
        assert np.array_equal(rho, plain)
        for b in range(batch):
            want = oracle.hs_dst(rho[b], centres[b % 3])
            assert abs(dist[b] - want) < 1e-13, (b, dist[b], want)
        others = [abs(dist[b] - oracle.hs_dst(rho[b], centres[(b + 1) % 3])) for b in range(batch)]
        assert min(others) > 1e-6  # the centres are told apart

    for physical in (True, False):
        dist, rho, st = outputs()
        eng.lin_dist_dev(cd, table, dist, physical=physical, rho=rho, status=st)
        check(dist, rho, st, eng.lin(counts, physical=physical))
    dist, rho, st = outputs()
    nit = torch.full((batch,), -1, dtype=torch.int32, device="cuda")
    eng.mle_dist_dev(cd, table, dist, rho=rho, nit=nit, status=st)
    plain, info = eng.mle(counts, return_info=True)
    check(dist, rho, st, plain)
    assert np.array_equal(nit.cpu().numpy(), info["nit"]) and np.all(info["nit"] >= 1)


def _freq_trials(s, k, batch, seed):
    rng = np.random.default_rng(seed)
    return rng.dirichlet(np.ones(k), (batch, s))


@pytest.mark.parametrize("batch", [259, 513])
@pytest.mark.parametrize("s,k,rows", [(5, 3, 7), (2, 512, 3)])
def test_moment_groups_of_256_trials_from_frequencies(qp, oracle, s, k, rows, batch):
    """moment_from_freq cuts the batch at 256 trials (dfreq + b0 M, dmean + b0, dvar + b0; the `part` and, for K > 256,
    `qpart` workspaces hold one group): B = 259 has one seam, 513 two and a last group of one trial.  (2, 512) has two
    pieces per setting, so qpart is in use.  Against oracle.l2_moments on the trials around each seam, at the tolerances of
    test_gpu_moments_large.check; those trials alone give the same bits as in the batch."""
    inv, ns, _ = make_inputs(s, k, rows, 1)
    freq = _freq_trials(s, k, batch, 6000 + batch + k)
    eng = qp.get_engine(1)
    mean, var = eng.moments_freq(freq, float(ns[0]), inv)
    around = sorted({0, 255, 256, 257, batch - 2, batch - 1})
    want = [oracle.l2_moments(freq[b], float(ns[0]), inv) for b in around]
    check_moments(mean[around], var[around], want, ("groups", s, k, batch))
    m1, v1 = eng.moments_freq(freq[around], float(ns[0]), inv)
    assert np.array_equal(m1, mean[around]) and np.array_equal(v1, var[around])
    lo_m, lo_v = eng.moments_freq(freq[:256], float(ns[0]), inv)
    hi_m, hi_v = eng.moments_freq(freq[256:], float(ns[0]), inv)
    differ = np.flatnonzero((np.concatenate([lo_m, hi_m]) != mean) | (np.concatenate([lo_v, hi_v]) != var))
    assert differ.size == 0, ("trials that differ from their piece:", differ[:8], "of", differ.size)


def test_moment_groups_of_256_trials_from_counts(qp, oracle):
    """qt_moment_batch above 8192 rows ((1100, 8): counts -> frequencies -> moment_from_freq) with B = 258: the three
    trials of test_gpu_moments_large's large_case sit at 0, 255, 256 and 257 (the first of them twice), so the oracle's
    cached values serve; the other 254 trials are draws of their own."""
    shape = (1100, 8, 6, 3)
    inv, ns, counts3, want3 = large_case(oracle, shape)
    rng = np.random.default_rng(6100)
    batch = 258
    p = rng.dirichlet(np.ones(shape[1]), (batch, shape[0]))
    counts = rng.multinomial(np.broadcast_to(ns, (batch, shape[0])), p).astype(np.int64)
    placed = {0: 0, 255: 1, 256: 2, 257: 0}
    for b, t in placed.items():
        counts[b] = counts3[t]
    eng = qp.get_engine(1)
    mean, var = eng.moments(counts, ns, inv)
    where = sorted(placed)
    check_moments(mean[where], var[where], [want3[placed[b]] for b in where], ("groups from counts", shape))
    lo_m, lo_v = eng.moments(counts[:256], ns, inv)
    hi_m, hi_v = eng.moments(counts[256:], ns, inv)
    assert np.array_equal(np.concatenate([lo_m, hi_m]), mean) and np.array_equal(np.concatenate([lo_v, hi_v]), var)
    assert mean[257] == mean[0] and var[257] == var[0]


def test_n3_kron_gemm_stripes_of_8192_processes(qp):
    """lifp_launch's kKronGemm path (n = 3, M % 4 != 0) runs its real GEMM in stripes of 8192 processes (grid.y <= 65535
    row tiles of 16: 8192 x 64 rows make 32768), with F + b0 R and T + b0 D D 2.  B = 8192 + 5 on the M = 218 POVM of
    test_n3_lifp_both_kernel_paths_against_the_factor_formula, the counts drawn on the device: the whole batch equals the
    calls on [0:8192] and [8192:] bit for bit, and processes 0, 8191, 8192 and B - 1 equal X = V_S^+ F V_P^+^T evaluated in
    NumPy with the engine's factors, at that test's 1e-11.  About 3 GB for a moment, on a private engine."""
    import torch

    from quantpy_amd import _capi

    g3 = load_golden("process3")
    np.random.seed(int(g3["Q0_seed"]))
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
    tmg.experiment(int(g3["Q0_shots"]), "proj-set")
    rows = np.asarray(tmg.tomographs[0].povm_matrix, dtype=np.float64).reshape(-1, 64) / 27.0
    rows = np.concatenate([rows[:-1]] + [rows[-1:] / 3] * 3)
    d, D, M, stripe = 8, 64, rows.shape[0], 8192
    assert M == 218
    batch = stripe + 5
    eng = qp.Engine(3)
    try:
        eng.set_povm(rows[None], 10000 * 27)
        eng.process_setup(np.stack([np.asarray(s.matrix, dtype=np.complex128) for s in tmg.input_basis.elements]))
        vs = np.empty((D, D), dtype=np.complex128)
        vp = np.empty((D, M), dtype=np.complex128)
        assert eng.lib.qt_process_get_factors(eng._h, vs.ctypes.data, vp.ctypes.data, _capi.QT_HOST_PTR) == 0
        gen = torch.Generator(device="cuda")
        gen.manual_seed(7001)
        counts = torch.randint(1, 4000, (batch, D, 1, M), dtype=torch.int64, device="cuda", generator=gen)
        whole = torch.empty((batch, D, D), dtype=torch.complex128, device="cuda")
        eng.lifp_dev(counts, whole, cptp=False)
        pieces = torch.empty((batch, D, D), dtype=torch.complex128, device="cuda")
        eng.lifp_dev(counts[:stripe], pieces[:stripe], cptp=False)
        eng.lifp_dev(counts[stripe:], pieces[stripe:], cptp=False)
        differ = torch.nonzero((torch.view_as_real(whole) != torch.view_as_real(pieces)).flatten(1).any(1)).flatten()
        assert differ.numel() == 0, ("processes that differ from their piece:", differ[:8].tolist(), "of", differ.numel())
        a, b, c, e = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), np.arange(d), indexing="ij")
        for k in (0, stripe - 1, stripe, batch - 1):
            ck = counts[k, :, 0, :].cpu().numpy()
            f = ck / ck.sum(axis=1, keepdims=True)
            x = vs @ f @ vp.T
            want = np.empty((D, D), dtype=np.complex128)
            want[(a * d + b).ravel(), (c * d + e).ravel()] = x[(a * d + c).ravel(), (e * d + b).ravel()]
            err = np.abs(whole[k].cpu().numpy() - want).max()
            assert err < 1e-11 * max(1.0, np.abs(want).max()), (k, err)
        del counts, whole, pieces
    finally:
        eng.close()
        torch.cuda.empty_cache()


def test_n2_dense_gemm_four_passes(qp, oracle):
    """lifp_launch's kDenseGemm path keeps a workgroup's operand slice for four passes once nblocks = ceil(B / 64) >= 64,
    i.e. B >= 4033.  B = 4100: nblocks = 65, four passes, 17 row blocks, the last with one block of 64 processes of which
    4 exist.  Whole against slices of 200 (the one-process-per-workgroup kernel) within 1e-12, against the default path
    through the Kronecker factors within 1e-11 (the bounds of the b2 = 2100 block of
    test_lifp_batched_gemm_path_matches_fused_kernel_and_oracle), and the oracle on processes of the first and last row
    block (1e-9, as there)."""
    np.random.seed(31)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.3, 2))
    tmg.experiment(5000, "proj-set")
    eng = tmg._engine()
    nset = tmg.results.shape[1]
    rng = np.random.default_rng(7100)
    batch = 4100
    assert (batch + 63) // 64 == 65
    probs = rng.dirichlet(np.full(4, 20.0), (batch, 16, nset))
    counts = rng.multinomial(5000, probs).astype(np.int64)
    eng.process_prefer_dense(True)
    try:
        big = eng.lifp(counts, cptp=False)
        ref = np.concatenate([eng.lifp(counts[lo:lo + 200], cptp=False) for lo in range(0, batch, 200)])
    finally:
        eng.process_prefer_dense(False)
    per = np.abs(big - ref).reshape(batch, -1).max(1)
    assert per.max() < 1e-12, ("processes off their slice:", np.flatnonzero(per >= 1e-12)[:8], per.max())
    assert np.abs(eng.lifp(counts, cptp=False) - big).max() < 1e-11
    ins = oracle.input_states("proj4", 2)
    a = oracle.measurement_matrix("proj-set", 2)
    for t in (0, 4031, 4032, 4095, 4096, batch - 1):
        assert np.abs(big[t] - oracle.lifp_estimate(counts[t], a, ins)).max() < 1e-9, t
