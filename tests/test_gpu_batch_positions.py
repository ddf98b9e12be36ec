"""GPU: batches whose members DIFFER, for the batched chain and process entries that the rest of the suite runs on single
trials or on copies of one trial: every trial / chain `b > 0` must find its own counts, starting point, proposal
increments and uniforms, and write its own rows of the outputs.  Each batch below is built from different true states or
channels, different starting points and different random streams, and is compared (a) with a plain NumPy run of the same
trial from the CPU oracle and (b) with the same trial launched alone, bit for bit where nothing is shared between trials.

The chains' inputs are chosen so that the comparison of accept flags is meaningful; the conditions are asserted here from
the oracle's run alone (no GPU number enters them):
  * the acceptance rate over the batch lies in [0.2, 0.8];
  * at half or more of the steps the chains that share a wavefront do not all decide alike;
  * |u_t - alpha_t| > 1e-9 at every step, so that no accept decision rests on rounding."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def qp():
    import quantpy_amd

    return quantpy_amd


def _ginibre(rng, d, rank=None):
    g = rng.standard_normal((d, rank or d)) + 1j * rng.standard_normal((d, rank or d))
    rho = g @ g.conj().T
    return rho / np.trace(rho)


def _check_chain_inputs(acc, margin, mates, what):
    """The three conditions of the module docstring on the oracle's flags acc (C, T) and margins |u - alpha| (C, T);
    `mates` = the leading chains that decide side by side."""
    rate = acc.mean()
    mixed = np.mean([0 < acc[:mates, t].sum() < min(mates, acc.shape[0]) for t in range(acc.shape[1])])
    assert 0.2 <= rate <= 0.8, (what, rate)
    assert mixed >= 0.5, (what, mixed)
    assert margin.min() > 1e-9, (what, margin.min())
    return rate, mixed, margin.min()


# ---- a. state chains, several per launch -------------------------------------------------------------------------
STATE_T = 30
STATE_SHOTS = 1000
# n: (chains, step, seed, chains deciding side by side, width of the uniforms).  n = 1: 16 chains per wavefront, n = 2: 4.
# n = 3 has one chain per wavefront, so the condition on mixed decisions is put to the four chains of the first workgroup.
# The reference's target is exp(-nll) with the frequencies normalised to sum 1 (state.py:222-229): it is so flat that with
# u ~ U[0, 1) nine proposals in ten are accepted whatever the step (n = 3: 96 %).  The kernel takes any u, so the uniforms
# are drawn from [1 - width, 1), where alpha = exp(f - f') lives, and accept and reject both happen.
STATE_CASES = {1: (70, 0.3, 101, 16, 0.1), 2: (21, 0.1, 102, 4, 0.1), 3: (5, 0.1, 103, 4, 0.1)}


def _state_batch(oracle, n):
    """Inputs of `STATE_CASES[n]` and the oracle's chains: (counts, x0, deltas, uniforms, step, chain, acc, margin)."""
    n_chain, step, seed, _, width = STATE_CASES[n]
    d = 2**n
    rng = np.random.default_rng(seed)
    povm = oracle.measurement_matrix("proj-set", n)
    np.random.seed(seed)
    counts, x0 = [], []
    for c in range(n_chain):  # alternating full-rank and rank-1 states, every one different
        rho = _ginibre(rng, d, rank=None if c % 2 == 0 else 1)
        counts.append(oracle.sample_counts(povm, oracle.bloch_from_matrix(rho), STATE_SHOTS))
        w = 0.1 + 0.3 * rng.random()
        x0.append(oracle.matrix_to_tril_vec((1 - w) * rho + w * _ginibre(rng, d)))
    counts, x0 = np.stack(counts).astype(np.int64), np.stack(x0)
    deltas = rng.standard_normal((n_chain, STATE_T, d * d))
    uniforms = 1.0 - width * rng.random((n_chain, STATE_T))
    chain = np.empty((n_chain, STATE_T, d * d))
    acc = np.empty((n_chain, STATE_T), dtype=np.int32)
    margin = np.empty((n_chain, STATE_T))
    for c in range(n_chain):
        chain[c], acc[c] = oracle.mhmc_state_chain(counts[c], povm, x0[c], deltas[c], uniforms[c], step)
        prob = oracle.NllProblem(counts[c], povm)
        x = x0[c]
        for t in range(STATE_T):  # the accept test of every step once more, for its margin
            xp = x + step * deltas[c, t]
            xp = xp / np.linalg.norm(xp)
            margin[c, t] = abs(uniforms[c, t] - np.exp(prob.nll(x) - prob.nll(xp)))
            x = chain[c, t]
    return counts, x0, deltas, uniforms, step, chain, acc, margin


@pytest.mark.parametrize("n", [1, 2, 3])
def test_state_chains_of_a_batch_match_the_oracle_and_themselves_alone(qp, oracle, n):
    """k_mhmc_state<n> with (n, C) = (1, 70), (2, 21), (3, 5): partial last wavefront and a second workgroup.  Every chain
    against oracle.mhmc_state_chain (flags identical, states to 1e-12) and against the same chain launched alone
    (np.array_equal: the kernel takes no wave-level decision, wave-mates that accept and reject at different steps
    cannot change a chain's bits)."""
    counts, x0, deltas, uniforms, step, want, want_acc, margin = _state_batch(oracle, n)
    _check_chain_inputs(want_acc, margin, STATE_CASES[n][3], f"state chains n={n}")
    eng = qp.get_engine(n)
    eng.set_povm(qp.generate_measurement_matrix("proj-set", n), np.ones(3**n) * STATE_SHOTS)
    chain, acc = eng.mhmc_state(counts, x0, deltas, uniforms, step)
    assert chain.shape == want.shape and acc.shape == want_acc.shape
    for c in range(counts.shape[0]):
        assert np.array_equal(acc[c], want_acc[c]), (n, c, acc[c], want_acc[c])
        err = np.abs(chain[c] - want[c]).max()
        assert err < 1e-12, (n, c, err)
    for c in range(counts.shape[0]):
        one, one_acc = eng.mhmc_state(counts[c], x0[c], deltas[c], uniforms[c], step)
        assert np.array_equal(one, chain[c]) and np.array_equal(one_acc, acc[c]), (n, c)


# ---- b. process chains, n = 1 and n = 2 --------------------------------------------------------------------------
PROC_T = 12
# n: (shots per setting, step, seed)
PROC_CASES = {1: (2000, 0.006, 201), 2: (2000, 0.0006, 202)}


def _channels(oracle, n, rng):
    """Three different channels as Choi matrices: depolarizing, amplitude damping (n = 1) / a unitary (n = 2), and a
    random channel of Kraus rank 2."""
    d = 2**n
    eye = np.eye(d)
    dep = oracle.choi_from_func(lambda e: 0.15 * np.trace(e) * eye / d + 0.85 * e, n)
    if n == 1:
        k0, k1 = np.sqrt(0.3) * np.array([[0, 1], [0, 0]]), np.diag([1.0, np.sqrt(0.7)])
        second = oracle.choi_from_func(lambda e: k0 @ e @ k0.conj().T + k1 @ e @ k1.conj().T, n)
    else:
        u, _ = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
        second = oracle.choi_from_func(lambda e: u @ e @ u.conj().T, n)
    k = rng.standard_normal((2, d, d)) + 1j * rng.standard_normal((2, d, d))
    w, v = np.linalg.eigh(sum(a.conj().T @ a for a in k))
    k = k @ ((v / np.sqrt(w)) @ v.conj().T)  # sum K^dagger K = 1
    third = oracle.choi_from_func(lambda e: sum(a @ e @ a.conj().T for a in k), n)
    return [dep, second, third]


def _process_counts(oracle, n, shots, seed):
    """(povm, input states (D, d, d), counts (3, D, S, K), the three true Choi matrices)."""
    rng = np.random.default_rng(seed)
    povm = oracle.measurement_matrix("proj-set", n)
    ins = oracle.input_states("proj4", n)
    chois = _channels(oracle, n, rng)
    np.random.seed(seed)
    counts = np.stack([np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(oracle.apply_choi(ch, s, n)), shots)
                                 for s in ins]) for ch in chois]).astype(np.int64)
    return povm, np.stack(ins), counts, chois


def _process_batch(oracle, n):
    """Inputs of `PROC_CASES[n]` and the NumPy chains: the proposal is P_CPTP(x + step * delta), accepted iff
    u <= exp(nll(x) - nll(x')) with nll = -sum n log(A x + 1e-12), as in oracle.mhmc_process_interval."""
    shots, step, seed = PROC_CASES[n]
    povm, ins, counts, chois = _process_counts(oracle, n, shots, seed)
    rng = np.random.default_rng(seed + 50)
    dim = 4**n
    oper = oracle.lifp_operator(list(ins), povm, counts[0, 0].sum(-1))
    x0 = np.stack([oracle.cptp_projection(oracle.lifp_estimate(c, povm, list(ins)), n) for c in counts])
    for start, truth in zip(x0, chois):  # (the sampled counts belong to these channels, in this layout)
        assert np.abs(start - truth).max() < 0.15
    deltas = rng.standard_normal((3, PROC_T, dim * dim))
    uniforms = rng.random((3, PROC_T))
    chain = np.empty((3, PROC_T, dim, dim), dtype=np.complex128)
    acc = np.empty((3, PROC_T), dtype=np.int32)
    margin = np.empty((3, PROC_T))
    for c in range(3):
        unnorm = counts[c].reshape(-1).astype(float)

        def logp(v):
            return np.sum(unnorm * np.log(oper @ v + 1e-12))  # = -nll, complex like the reference's

        x = oracle.mat2vec(x0[c])
        for t in range(PROC_T):
            xp = oracle.mat2vec(oracle.cptp_projection(oracle.vec2mat(x + step * deltas[c, t]), n))
            alpha = np.exp(logp(xp) - logp(x))
            ok = (uniforms[c, t], 0.0) <= (alpha.real, alpha.imag)  # NumPy orders complex numbers lexicographically
            margin[c, t] = abs(uniforms[c, t] - alpha.real)
            if ok:
                x = xp
            chain[c, t] = oracle.vec2mat(x)
            acc[c, t] = ok
    return povm, ins, counts, x0, deltas, uniforms, step, chain, acc, margin


@pytest.fixture(scope="module")
def process_batches(oracle):
    return {n: _process_batch(oracle, n) for n in (1, 2)}


@pytest.mark.parametrize("n", [1, 2])
def test_process_chains_of_a_batch_match_numpy_and_themselves_alone(qp, oracle, process_batches, n):
    """k_mhmc_process<4 / 16> with C = 3: every b-dependent index (counts, choi_init, deltas, uniforms, chain_out,
    accepted).  Flags identical to the NumPy chain, Choi matrices to 1e-8; each chain equal to itself alone bit for bit
    (one workgroup per chain, nothing shared)."""
    povm, ins, counts, x0, deltas, uniforms, step, want, want_acc, margin = process_batches[n]
    _check_chain_inputs(want_acc, margin, 3, f"process chains n={n}")
    eng = qp.get_engine(n)
    eng.set_povm(povm, counts[0, 0].sum(-1).astype(float))
    eng.process_setup(ins)
    chain, acc = eng.mhmc_process(counts, x0, deltas, uniforms, step)
    dim = 4**n
    assert chain.shape == (3, PROC_T, dim, dim) and acc.shape == (3, PROC_T)
    for c in range(3):
        assert np.array_equal(acc[c], want_acc[c]), (n, c, acc[c], want_acc[c])
        err = np.abs(chain[c] - want[c]).max()
        assert err < 1e-8, (n, c, err)
    for c in range(3):
        one, one_acc = eng.mhmc_process(counts[c], x0[c], deltas[c], uniforms[c], step)
        assert one.shape == (PROC_T, dim, dim) and one_acc.shape == (PROC_T,)
        assert np.array_equal(one, chain[c]) and np.array_equal(one_acc, acc[c]), (n, c)


# ---- c. process chains, n = 3 ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n3_processes(qp):
    """Two three-qubit tomographs: the depolarizing one of test_n3_mhmc_process_interval_matches_the_reference, and a
    depolarized Walsh-Hadamard channel.  -> (the first tomograph, counts (2, 64, 27, 8))."""
    np.random.seed(31)
    first = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
    first.experiment(10000, "proj-set")
    np.random.seed(32)
    second = qp.ProcessTomograph(qp.channel.depolarize(qp.channel.walsh_hadamard(3), 0.2))
    second.experiment(10000, "proj-set")
    counts = np.stack([first.results, second.results]).astype(np.int64)
    assert not np.array_equal(counts[0], counts[1])
    return first, counts


def test_n3_process_chains_of_a_batch_equal_the_chains_alone(n3_processes):
    """The factored chain path with C = 2, T = 3: k_fwd64_nll on C * nt workgroups, fcur / fpart behind C * ws_doubles,
    k_mhmc64_propose / k_mhmc64_decide on C workgroups, project64 on C matrices.  The oracle's dense operator is not
    affordable and the one-chain path is pinned to the reference already, so: both chains and their flags equal the two
    one-chain launches bit for bit."""
    tmg, counts = n3_processes
    eng = tmg._engine()  # (POVM, shots and input states are the same for both tomographs)
    x0 = eng.lifp(counts, cptp=True)
    assert np.abs(x0[0] - x0[1]).max() > 0.05
    rng = np.random.default_rng(303)
    deltas = rng.standard_normal((2, 3, 4096))
    uniforms = rng.random((2, 3))
    step = 1e-5  # (the step at which the reference's own chain on chain 0's counts accepted half its proposals)
    chain, acc = eng.mhmc_process(counts, x0, deltas, uniforms, step)
    assert chain.shape == (2, 3, 64, 64) and acc.shape == (2, 3) and np.isfinite(chain.view(np.float64)).all()
    print(f"n = 3 process chains: accepted {acc.tolist()}")
    for c in range(2):
        one, one_acc = eng.mhmc_process(counts[c], x0[c], deltas[c], uniforms[c], step)
        assert np.array_equal(one_acc, acc[c]), (c, one_acc, acc[c])
        assert np.array_equal(one, chain[c]), (c, np.abs(one - chain[c]).max())
        # a chain that moved went to a CPTP proposal of its own increments; one that stayed is at its own start
        for t in range(3):
            prev = x0[c] if t == 0 else chain[c, t - 1]
            assert np.array_equal(chain[c, t], prev) != bool(acc[c, t]), (c, t)


# ---- d. 'pgdb' on distinct batches -------------------------------------------------------------------------------
PGDB_SHOTS = (30, 300, 3000)


def _pgdb_counts(oracle, n):
    """Three trials from the three channels of `_channels`, measured with 30, 300 and 3000 shots per setting (raw counts
    are the weights of 'pgdb', and no total is registered per trial)."""
    parts = [_process_counts(oracle, n, shots, 240 + n) for shots in PGDB_SHOTS]
    povm, ins = parts[0][:2]
    return povm, ins, np.stack([part[2][k] for k, part in enumerate(parts)])


@pytest.mark.parametrize("stop", ["reference", "converged"])
@pytest.mark.parametrize("n", [1, 2])
def test_pgdb_trials_of_a_batch_equal_the_trials_alone(qp, oracle, n, stop):
    """k_pgdb_batch<4 / 16> with B = 3 different channels and shot numbers, n_iter = 3: Choi, iters and status of every
    trial equal the single-trial call bit for bit (the single-trial path is pinned to the oracle and the golden files
    elsewhere), and the trials differ from one another.

    What "differ" can mean here: the reference's loop (process.py:291-308, every quirk kept) hardly depends on the data.
    From the fully mixed start its trial point c - g / mu is ~1e5 in size, the projected direction is the TP correction of
    the start plus rounding noise, and the backtracking either takes it whole (few shots) or shrinks the step to ~1e-16
    (many shots); the reference's stop rule then returns the start itself or the start plus that noise.  The oracle gives
    the same picture (differences between these trials from 1e-43 to 0.25).  So two trials count as different when their
    (Choi, iters) are not the same bits -- which is all that the comparison with the single calls needs in order to tell a
    trial that read its neighbour's counts."""
    povm, ins, counts = _pgdb_counts(oracle, n)
    assert counts.shape[0] == 3 and [int(c[0, 0].sum()) for c in counts] == list(PGDB_SHOTS)
    eng = qp.get_engine(n)
    eng.set_povm(povm, np.ones(3**n) * PGDB_SHOTS[0])
    eng.process_setup(ins)
    choi, iters, status = eng.pgdb(counts, n_iter=3, stop=stop, return_iters=True, return_status=True)
    assert choi.shape == (3, 4**n, 4**n) and iters.shape == (3,) and status.shape == (3,)
    print(f"pgdb n={n} {stop}: iters {iters.tolist()} status {status.tolist()} differences "
          f"{[float(np.abs(choi[a] - choi[b]).max()) for a, b in ((0, 1), (0, 2), (1, 2))]}")
    assert list(status) == [0, 0, 0]
    for b in range(3):
        one, one_it, one_st = eng.pgdb(counts[b], n_iter=3, stop=stop, return_iters=True, return_status=True)
        assert np.array_equal(one, choi[b]), (n, stop, b, np.abs(one - choi[b]).max())
        assert one_it == iters[b] and one_st == status[b], (n, stop, b)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not (np.array_equal(choi[a], choi[b]) and iters[a] == iters[b]), (n, stop, a, b)


def test_n3_pgdb_trials_of_a_batch_equal_the_trials_alone(n3_processes):
    """The factored 'pgdb' (k_pgdb64_grad / project64 / k_pgdb64_step) with B = 2, n_iter = 2, stop='converged', and
    qt_pgdb_pieces with B = 2 at two different points: everything equal to the B = 1 calls bit for bit."""
    tmg, counts = n3_processes
    eng = tmg._engine()  # (POVM, shots and input states are the same for both tomographs)
    choi, iters, status = eng.pgdb(counts, n_iter=2, stop="converged", return_iters=True, return_status=True)
    assert np.isfinite(choi.view(np.float64)).all() and list(status) == [0, 0]
    points = eng.lifp(counts, cptp=True)
    probas, grad, proj = eng.pgdb_pieces(counts, points)
    assert probas.shape == (2, 64 * 216) and grad.shape == (2, 64, 64) and proj.shape == (2, 64, 64)
    for b in range(2):
        one, one_it, one_st = eng.pgdb(counts[b], n_iter=2, stop="converged", return_iters=True, return_status=True)
        assert np.array_equal(one, choi[b]), (b, np.abs(one - choi[b]).max())
        assert one_it == iters[b] and one_st == status[b], b
        p1, g1, x1 = eng.pgdb_pieces(counts[b], points[b])
        assert np.array_equal(p1, probas[b]) and np.array_equal(g1, grad[b]) and np.array_equal(x1, proj[b]), b
    assert not np.array_equal(choi[0], choi[1]) and np.abs(probas[0] - probas[1]).max() > 1e-3


# ---- e. make_feasible in wavefronts that mix positive-definite and clipped trials ---------------------------------
def _mixed_lin_batch(oracle, n, n_trials):
    """Counts (B, S, K), equal shots over the settings of a trial: even trials from a full-rank state with many shots
    (unclipped linear inversion positive definite), odd ones from a rank-1 state with 3 .. 50 shots (it is not).  ->
    (povm, counts, is_pd (B,))."""
    d = 2**n
    rng = np.random.default_rng(500 + n)
    povm = oracle.measurement_matrix("proj-set", n)
    np.random.seed(510 + n)
    counts, is_pd = [], []
    for b in range(n_trials):
        pd = b % 2 == 0
        while True:
            if pd:
                rho = 0.5 * _ginibre(rng, d) + 0.5 * np.eye(d) / d
                c = oracle.sample_counts(povm, oracle.bloch_from_matrix(rho), int(rng.integers(20000, 100000)))
            else:
                c = oracle.sample_counts(povm, oracle.bloch_from_matrix(_ginibre(rng, d, rank=1)), int(rng.integers(3, 51)))
            low = np.linalg.eigvalsh(oracle.lin_estimate(c, povm, physical=False)).min()
            if (low > 1e-3) if pd else (low < -1e-3):  # well on its side of the Cholesky test
                break
        counts.append(c)
        is_pd.append(pd)
    return povm, np.stack(counts).astype(np.int64), np.array(is_pd)


@pytest.mark.parametrize("n,n_trials", [(1, 70), (2, 21)])
def test_make_feasible_in_mixed_wavefronts(qp, oracle, n, n_trials):
    """Small<n>::make_feasible where every wavefront (16 trials at n = 1, 4 at n = 2; the last one partial) holds trials
    that pass the Cholesky test and trials that need the clip: `!__all(ok)`, the Jacobi loop until the whole wave has
    converged, the selection `if (!ok)` per trial."""
    povm, counts, is_pd = _mixed_lin_batch(oracle, n, n_trials)
    eng = qp.get_engine(n)
    eng.set_povm(povm, np.ones(3**n) * 1000)  # (equal shots per setting: any trial's totals are proportional to these)
    got = eng.lin(counts, physical=True)
    for b in range(n_trials):
        want = oracle.lin_estimate(counts[b], povm)
        assert np.abs(got[b] - want).max() < 1e-12, (n, b, np.abs(got[b] - want).max())
        assert abs(np.trace(got[b]) - 1) < 1e-13 and np.linalg.eigvalsh(got[b]).min() > 0, (n, b)
        if is_pd[b]:  # r / tr whatever the rest of the wave does
            assert np.array_equal(eng.lin(counts[b : b + 1], physical=True)[0], got[b]), (n, b)


@pytest.mark.parametrize("n,n_trials", [(1, 70), (2, 21)])
def test_chol_param_status_of_one_bad_matrix_per_wavefront(qp, oracle, n, n_trials):
    """k_chol_param<n> on a batch in which exactly one matrix of every wavefront is not positive definite: status 1
    there and 0 elsewhere, and the others' parameters are the oracle's to 1e-13."""
    d = 2**n
    per_wave = 64 // (d * d)
    rng = np.random.default_rng(520 + n)
    mats = np.stack([_ginibre(rng, d) for _ in range(n_trials)])
    bad = [int(rng.integers(w, min(w + per_wave, n_trials))) for w in range(0, n_trials, per_wave)]
    for b in bad:
        w, u = np.linalg.eigh(mats[b])
        w[int(rng.integers(d))] *= -1.0  # one negative eigenvalue
        m = (u * w) @ u.conj().T
        mats[b] = (m + m.conj().T) / 2
    eng = qp.get_engine(n)
    eng.set_povm(oracle.measurement_matrix("proj-set", n), np.ones(3**n) * 1000)
    x, status = eng.chol_param(mats)
    assert status.tolist() == [1 if b in bad else 0 for b in range(n_trials)]
    for b in range(n_trials):
        if b not in bad:
            err = np.abs(x[b] - oracle.matrix_to_tril_vec(mats[b])).max()
            assert err < 1e-13, (n, b, err)
