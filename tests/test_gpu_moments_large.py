"""GPU: the moment sums of MomentInterval above 8192 POVM rows and from real-valued frequencies -- k_moment_cols /
k_moment_finish behind qt_moment_batch (S K > 8192) and qt_moment_freq_batch (any size).  The yardstick is
oracle.l2_moments, the reference's fourteen einsums (stats.py:21-47 with the weights of interval.py:88); the tolerances
are those of test_gpu_moments.test_moment_kernel_on_arbitrary_shapes: 1e-12 relative on the mean, 1e-9 relative plus
1e-14 mean^2 on the variance.  Inputs are built as that test builds them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LARGE = [(1100, 8, 6, 3), (41, 216, 5, 2), (3, 3000, 4, 2)]  # S K = 8800, 8856, 9000: above the one-workgroup kernels
SMALL = [(5, 3, 7, 9), (1, 6, 4, 5), (35, 31, 10, 6), (81, 16, 256, 3), (144, 4, 256, 10), (2, 512, 3, 2)]


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def make_inputs(s, k, rows, batch):
    rng = np.random.default_rng(s * 1000 + k)
    inv = rng.standard_normal((rows, s * k)) * 0.1
    ns = rng.integers(20, 60, s)
    ns[0] = 37
    counts = np.stack([np.stack([rng.multinomial(int(ns[i]), rng.dirichlet(np.ones(k))) for i in range(s)]) for _ in range(batch)])
    return inv, ns, counts


_LARGE_CASES = {}


def large_case(oracle, shape):
    """Inputs and the oracle's moments per trial of one LARGE shape, computed once per session and left unchanged."""
    if shape not in _LARGE_CASES:
        inv, ns, counts = make_inputs(*shape)
        want = [oracle.l2_moments(c / ns[:, None], float(ns[0]), inv) for c in counts]
        _LARGE_CASES[shape] = (inv, ns, counts, want)
    return _LARGE_CASES[shape]


def check(got_mean, got_var, want, where):
    for b, (m0, v0) in enumerate(want):
        print(where, b, "mean", got_mean[b], m0, "var", got_var[b], v0)
        assert abs(got_mean[b] - m0) <= 1e-12 * abs(m0), (where, b, got_mean[b], m0)
        assert abs(got_var[b] - v0) <= 1e-9 * abs(v0) + 1e-14 * m0 * m0, (where, b, got_var[b], v0)


@pytest.mark.parametrize("shape", LARGE)
def test_integer_counts_above_8192_rows(qp, oracle, shape):
    """qt_moment_batch above its old limit.  (1100, 8): 35 column blocks of 32 settings, the last of 12, by 29 runs of
    settings; (41, 216): one setting per block, 216 of its 256 lanes in use, K neither a power of two nor a divisor of
    256; (3, 3000): K above the column block, every Q_ab summed from twelve pieces by the finishing kernel."""
    inv, ns, counts, want = large_case(oracle, shape)
    mean, var = qp.get_engine(1).moments(counts, ns, inv)
    check(mean, var, want, shape)


@pytest.mark.parametrize("s,k,rows,batch", SMALL)
def test_frequency_entry_on_the_small_shapes(qp, oracle, s, k, rows, batch):
    """qt_moment_freq_batch takes the new kernels at every size: the shapes of the arbitrary-shapes test, once with
    f = counts / ns and once with frequencies that no integer counts give (Dirichlet rows, passed as counts = f ns, which
    Engine.moments must send to this entry instead of raising TypeError).  Column blocks: (35, 31) has five of 8 settings,
    the last of 3; (81, 16) six of 16, the last of 1; (144, 4) three of 64, the last of 16; (2, 512) two pieces per
    setting.  No batch size here is a multiple of the four trials of a workgroup."""
    inv, ns, counts = make_inputs(s, k, rows, batch)
    eng = qp.get_engine(1)
    freq = counts / ns[:, None]
    mean, var = eng.moments_freq(freq, float(ns[0]), inv)
    check(mean, var, [oracle.l2_moments(f, float(ns[0]), inv) for f in freq], ("counts / ns", s, k))
    rng = np.random.default_rng(7 + s * 1000 + k)
    real = rng.dirichlet(np.ones(k), (batch, s)) * ns[:, None]
    assert not np.all(np.mod(real, 1) == 0)
    mean, var = eng.moments(real, ns, inv)
    check(mean, var, [oracle.l2_moments(c / ns[:, None], float(ns[0]), inv) for c in real], ("real-valued", s, k))


def test_bits_do_not_depend_on_the_batch_the_call_or_the_entry(qp):
    """At (1100, 8, 6): trial 1 alone = trial 1 in the batch, two identical calls agree, and the integer entry agrees
    with the frequency entry fed counts / ns -- all bit for bit."""
    inv, ns, counts = make_inputs(*LARGE[0])
    eng = qp.get_engine(1)
    mean, var = eng.moments(counts, ns, inv)
    m1, v1 = eng.moments(counts[1], ns, inv)
    assert m1 == mean[1] and v1 == var[1]
    mean2, var2 = eng.moments(counts, ns, inv)
    assert np.all(mean2 == mean) and np.all(var2 == var)
    mean3, var3 = eng.moments_freq(counts / ns[:, None], float(ns[0]), inv)
    assert np.all(mean3 == mean) and np.all(var3 == var)


def test_integer_counts_up_to_8192_rows_keep_their_bits(qp):
    """qt_moment_batch at S K <= 8192 launches what it launched before the frequency kernels existed.  The two numbers
    are eng.moments of trial 0 of the (35, 31, 10) inputs (1085 rows: k_moment_batch<1, 32>) as built from commit 81c1084
    ("Specialise the n <= 3 MLE kernels on the six-projector POVM shape") on an MI355X."""
    inv, ns, counts = make_inputs(35, 31, 10, 1)
    mean, var = qp.get_engine(1).moments(counts[0], ns, inv)
    assert float(mean).hex() == "0x1.683b23aefd7f8p-4" and float(var).hex() == "0x1.9ed7731c59218p-10", (float(mean).hex(), float(var).hex())


def matrix_form(inv, freq, n_trials, k):
    """The matrix form of qt_ops.h's comment in float64 on the GPU with torch: W = P^T P, U[a][c] = sum_i f_ai W[(a,i)][c],
    Q_ab = sum_j U[a][(b,j)] f_bj and the five sums."""
    import torch

    p = torch.as_tensor(np.ascontiguousarray(inv, dtype=np.float64), device="cuda")
    f = torch.as_tensor(np.ascontiguousarray(freq, dtype=np.float64).reshape(-1), device="cuda")
    m = f.numel()
    s = m // k
    w = torch.matmul(p.T, p)
    u = (w * f[:, None]).reshape(s, k, m).sum(1)
    q = (u * f[None, :]).reshape(s, s, k).sum(2)
    uuf = (u * u * f[None, :]).sum()
    wwf = torch.dot(f, torch.mv(w * w, f))
    t_d = torch.dot(torch.diagonal(w), f)
    q2, tr_q = (q * q).sum(), torch.trace(q)
    first = (t_d - tr_q) / n_trials
    second = ((tr_q - t_d) ** 2 + 2 * q2 - 4 * uuf + 2 * wwf) / n_trials**2
    return float(first), float(second - first * first)


def test_matrix_form_equals_the_oracle(oracle):
    """The independent check of the three-qubit process below, validated where the oracle is affordable: (35, 31, 10)."""
    inv, ns, counts = make_inputs(35, 31, 10, 1)
    freq = counts[0] / ns[:, None]
    m0, v0 = oracle.l2_moments(freq, float(ns[0]), inv)
    m1, v1 = matrix_form(inv, freq, float(ns[0]), 31)
    check([m1], [v1], [(m0, v0)], "matrix form")


def test_three_qubit_process_end_to_end(qp):
    """MomentInterval on a three-qubit ProcessTomograph with 'proj-set': 64 input states x 27 settings x 8 outcomes =
    13 824 rows, a 4096 x 13 824 left inverse and a 1.5 GB W.  Radii finite and increasing; radii_batch of two count tensors
    = the two single-tomograph calls (rtol 1e-12); mean and variance against the matrix form above.  One test on purpose:
    every MomentInterval call at this size rebuilds the design matrix and its left inverse (0.6 s each, four of them here:
    2.4 s measured on an MI355X, split in DESIGN.md section 8), and it must not be cut below 8193 rows."""
    np.random.seed(20261017)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
    tmg.experiment(1000, "proj-set")
    cls = np.array([0.5, 0.9, 0.99])
    itv = qp.MomentInterval(tmg)
    radii = itv(cls)[0]
    assert np.all(np.isfinite(radii)) and np.all(np.diff(radii) > 0), radii
    first = tmg.results
    _, n_meas, own, inv = itv._design()
    assert own.shape == (64 * 27, 8) and inv.shape == (4096, 13824)
    m1, v1 = matrix_form(inv, own / n_meas[:, None], float(n_meas[0]), 8)
    check([itv.mean], [itv.variance], [(m1, v1)], "three-qubit process")
    del inv
    tmg.experiment(1000, "proj-set")
    second = tmg.results
    radii2 = qp.MomentInterval(tmg)(cls)[0]
    batch = qp.MomentInterval(tmg).radii_batch(np.stack([first, second]), cls)
    assert np.allclose(batch[0], radii, rtol=1e-12) and np.allclose(batch[1], radii2, rtol=1e-12), (batch, radii, radii2)


def test_real_valued_results_through_the_class(qp, oracle):
    """A one-qubit StateTomograph whose results are the expected counts 1000 p (the reference divides in floating point
    and takes them, interval.py:74): MomentInterval's radii = the oracle's, rtol 1e-10."""
    rng = np.random.default_rng(11)
    g = rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2))
    rho = g @ g.conj().T
    rho /= np.trace(rho)
    tmg = qp.StateTomograph(qp.Qobj(rho))
    tmg.experiment(1000, "proj-set")
    povm = np.asarray(tmg.povm_matrix)
    tmg.results = 1000 * np.einsum("ijk,k->ij", povm, oracle.bloch_from_matrix(rho)) * 2
    assert not np.all(np.mod(tmg.results, 1) == 0)
    cls = np.array([0.5, 0.9, 0.99])
    got = qp.MomentInterval(tmg)(cls)[0]
    assert np.allclose(got, oracle.moment_radii(tmg.results, povm, cls), rtol=1e-10)
