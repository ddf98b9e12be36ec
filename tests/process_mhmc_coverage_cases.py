"""Shared by tests/test_process_mhmc_coverage_host.py and tests/test_gpu_process_mhmc_coverage.py: the batches of process
tomographies the GPU tests run their chains on, and the chain restated in NumPy on the CPU oracle (what the Philox seeds
of the GPU tests were searched with).  The host build of the draws is `mhmc_coverage_cases.build_host_draws`, which takes
the vector length as a parameter."""
import numpy as np

from mhmc_coverage_cases import build_host_draws  # noqa: F401  (re-exported)

SHOTS = 2000
STEPS = {1: 0.006, 2: 0.0006}  # proposal step per n: those of test_gpu_batch_positions.py at the same number of shots
SETTINGS = {"thinned": (3, 7, 2), "plain": (0, 40, 1)}  # burn_steps, n_points, thinning
CASES = [(1, 1), (1, 5), (2, 3)]  # (n, chains)


def channels(oracle, n, count, rng):
    """`count` different channels as Choi matrices, cycling through three kinds with their own parameters: depolarizing,
    amplitude damping (n = 1) / a random unitary (n = 2), and a random channel of Kraus rank 2."""
    d = 2**n
    eye = np.eye(d)
    out = []
    for c in range(count):
        kind = c % 3
        if kind == 0:
            p = 0.15 + 0.1 * (c // 3)
            out.append(oracle.choi_from_func(lambda e, p=p: p * np.trace(e) * eye / d + (1 - p) * e, n))
        elif kind == 1 and n == 1:
            g = 0.3 + 0.2 * (c // 3)
            k0, k1 = np.sqrt(g) * np.array([[0, 1], [0, 0]]), np.diag([1.0, np.sqrt(1 - g)])
            out.append(oracle.choi_from_func(lambda e, k0=k0, k1=k1: k0 @ e @ k0.conj().T + k1 @ e @ k1.conj().T, n))
        elif kind == 1:
            u, _ = np.linalg.qr(rng.standard_normal((d, d)) + 1j * rng.standard_normal((d, d)))
            out.append(oracle.choi_from_func(lambda e, u=u: u @ e @ u.conj().T, n))
        else:
            k = rng.standard_normal((2, d, d)) + 1j * rng.standard_normal((2, d, d))
            w, v = np.linalg.eigh(sum(a.conj().T @ a for a in k))
            k = k @ ((v / np.sqrt(w)) @ v.conj().T)  # sum K^dagger K = 1
            out.append(oracle.choi_from_func(lambda e, k=k: sum(a @ e @ a.conj().T for a in k), n))
    return out


def trial_batch(oracle, n, chains, seed):
    """`chains` process tomographies ('proj-set', 'proj4', SHOTS per setting), each of its own channel: (povm, input states
    (D, d, d), counts (C, D, S, K) int64, the true Choi matrices (C, D, D), the starting points (C, D, D)) -- every chain
    starts from the CPTP-projected 'lifp' estimate of its own counts (CPU oracle)."""
    rng = np.random.default_rng(seed)
    povm = oracle.measurement_matrix("proj-set", n)
    ins = oracle.input_states("proj4", n)
    chois = channels(oracle, n, chains, rng)
    np.random.seed(seed)
    counts = np.stack([np.stack([oracle.sample_counts(povm, oracle.bloch_from_matrix(oracle.apply_choi(ch, s, n)), SHOTS)
                                 for s in ins]) for ch in chois]).astype(np.int64)
    x0 = np.stack([oracle.cptp_projection(oracle.lifp_estimate(c, povm, list(ins)), n) for c in counts])
    # (np.stack keeps the column-major layout the oracle's vec2mat views have: the arrays go to torch as they are)
    return povm, np.stack(ins), counts, np.ascontiguousarray(np.stack(chois)), np.ascontiguousarray(x0)


def numpy_chain(oracle, n, povm, ins, counts, x0, deltas, uniforms, step):
    """One chain in NumPy as test_gpu_batch_positions.py restates it: the proposal is P_CPTP(x + step * delta), accepted
    iff u <= exp(nll(x) - nll(x')) with nll = -sum n log(A x + 1e-12).  -> (chain (T, D, D), accepted (T,))."""
    oper = oracle.lifp_operator(list(ins), povm, counts[0].sum(-1))
    unnorm = counts.reshape(-1).astype(float)

    def logp(v):
        return np.sum(unnorm * np.log(oper @ v + 1e-12))

    x = oracle.mat2vec(x0)
    chain = np.empty((len(uniforms),) + x0.shape, dtype=np.complex128)
    acc = np.empty(len(uniforms), dtype=np.int64)
    for t, u in enumerate(uniforms):
        xp = oracle.mat2vec(oracle.cptp_projection(oracle.vec2mat(x + step * deltas[t]), n))
        alpha = np.exp(logp(xp) - logp(x))
        ok = (u, 0.0) <= (alpha.real, alpha.imag)  # NumPy orders complex numbers lexicographically
        if ok:
            x = xp
        chain[t], acc[t] = oracle.vec2mat(x), ok
    return chain, acc


def median_off_samples(dist):
    """A threshold in the middle of one chain's distances and on none of them."""
    s = np.unique(dist)
    return 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2]) if len(s) > 1 else 1.5 * s[0] + 1e-3


def thresholds(delta, dist):
    """The trial's own delta for the odd chains, the nudged median of the chain's distances for the even ones."""
    return np.array([delta[c] if c % 2 else median_off_samples(dist[c]) for c in range(len(delta))])


def batch_seed(n, chains):
    return 500 + 10 * n + chains


def cpu_study(oracle, host_draws, n, chains, draw_seed, setting):
    """The unfused study of a case on the CPU (host draws, `numpy_chain`, oracle.hs_dst of the real parts): (kept
    distances (C, n_points), accepted post-burn (C,), thresholds (C,)).  The search of the Philox seeds ran this."""
    burn, n_points, thinning = SETTINGS[setting]
    povm, ins, counts, chois, x0 = trial_batch(oracle, n, chains, batch_seed(n, chains))
    total = burn + n_points * thinning
    deltas, uniforms = host_draws(draw_seed, 0, chains, 0, total, 16**n)
    dist = np.empty((chains, n_points))
    acc = np.empty(chains, dtype=np.int64)
    for c in range(chains):
        chain, flags = numpy_chain(oracle, n, povm, ins, counts[c], x0[c], deltas[c], uniforms[c], STEPS[n])
        kept = chain[burn::thinning][:n_points].real
        dist[c] = [oracle.hs_dst(m, x0[c]) for m in kept]
        acc[c] = flags[burn:].sum()
    delta = np.array([oracle.hs_dst(x0[c], chois[c]) for c in range(chains)])
    return dist, acc, thresholds(delta, dist)
