"""GPU: the state intervals and the bootstrap coverage study in the trace distance and the infidelity, on the engine's
batched distances (Engine.metric_dist / metric_dist_dev) instead of one scipy.linalg.sqrtm per resample on the host.

* BootstrapStateInterval(dst='trace' / 'if') takes the one-pass, sharded path: counts as before, distances within 1e-7
  (trace) / 1e-6 (infidelity) of `tmg.dst(Qobj(r), centre)` on the host -- the bounds of tests/test_gpu_metric_dist.py
  against the reference's own sqrtm -- and the same bits whatever the chunking of the density-matrix workspace.
* MHMCStateInterval: the chain is untouched, the distances are within the same bounds of the host loop.
* metrics.get_CL_list_state_boot: dst='hs' is get_CL_list_state(interval='boot') bit for bit; 'trace' / 'if' against the
  documented keying, redrawn resample by resample and measured on the host."""
import numpy as np
import pytest
from scipy.interpolate import interp1d

pytestmark = pytest.mark.gpu

TOL = {"trace": 1e-7, "if": 1e-6}
LEVELS = np.array([0.05, 0.5, 0.9, 0.95])
N_POINTS = 9
SHOTS = 10**4


def _ginibre_state(n, seed):
    """A full-rank state: G G^dagger / Tr of a complex Ginibre matrix."""
    import quantpy_amd as qp

    g = np.random.default_rng(seed)
    m = g.standard_normal((2**n, 2**n)) + 1j * g.standard_normal((2**n, 2**n))
    rho = m @ m.conj().T
    return qp.Qobj(rho / np.trace(rho).real)


def _measured(n, dst, method, seed=31):
    """A tomograph with results and a point estimate, and np.random's state behind them."""
    import quantpy_amd as qp

    tmg = qp.StateTomograph(_ginibre_state(n, 60 + n), dst)
    np.random.seed(seed)
    tmg.experiment(SHOTS)
    tmg.point_estimate(method)
    return tmg, np.random.get_state()


def _host_distances(tmg, counts, centre, method):
    import quantpy_amd as qp

    boot = qp.StateTomograph(centre, tmg.dst)
    boot.povm_matrix, boot.n_measurements = tmg.povm_matrix, tmg.n_measurements
    rho, _ = boot.point_estimate_batch(counts, method=method)
    return np.array([tmg.dst(qp.Qobj(r), centre) for r in rho], dtype=np.float64)


# ---- 4. BootstrapStateInterval -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dst", ["trace", "if"])
@pytest.mark.parametrize("method", ["lin", "mle"])
@pytest.mark.parametrize("n", [2, 3])
def test_bootstrap_interval_one_pass(n, method, dst):
    import quantpy_amd as qp
    from quantpy_amd.distributed import ShardedSample

    tmg, stream = _measured(n, dst, method)
    iv = qp.BootstrapStateInterval(tmg, n_points=N_POINTS, method=method)
    got, levels = iv(LEVELS)
    assert isinstance(iv.sample, ShardedSample)
    centre = tmg.reconstructed_state
    np.random.set_state(stream)
    want_counts = qp.StateTomograph(centre, dst).experiment_batch(tmg.n_measurements, tmg.povm_matrix, N_POINTS)
    assert iv.boot_counts.shape == (N_POINTS,) + tmg.results.shape and np.array_equal(iv.boot_counts, want_counts)
    host = _host_distances(tmg, want_counts, centre, method)
    print(n, method, dst, "engine", iv.boot_dist, "host", host, "max diff", np.abs(iv.boot_dist - host).max())
    assert iv.boot_dist.shape == (N_POINTS,) and np.abs(iv.boot_dist - host).max() <= TOL[dst]
    assert (iv.boot_dist > 1e-5).all()  # resamples at 10^4 shots: nowhere near the 1e-15 rule
    assert np.array_equal(got, interp1d(np.linspace(0, 1, N_POINTS), np.sort(iv.boot_dist))(LEVELS))
    assert np.array_equal(iv.cl_to_dist.y, np.sort(iv.boot_dist))
    # three chunks of three trials through the density-matrix workspace: the same bits
    tmg2, _ = _measured(n, dst, method)
    chunked = qp.BootstrapStateInterval(tmg2, n_points=N_POINTS, method=method)
    chunked._CHUNK_BYTES = 3 * 16 * 4**n
    chunked.setup()
    assert np.array_equal(chunked.boot_counts, want_counts)
    assert np.array_equal(chunked.boot_dist.view(np.int64), iv.boot_dist.view(np.int64))


@pytest.mark.parametrize("dst", ["trace", "if"])
def test_bootstrap_interval_device_sampler(dst):
    import quantpy_amd as qp
    from quantpy_amd.distributed import ShardedSample

    tmg, _ = _measured(2, dst, "lin")
    iv = qp.BootstrapStateInterval(tmg, n_points=N_POINTS, method="lin", sampler="device", seed=5)
    iv.setup()
    assert isinstance(iv.sample, ShardedSample)
    counts = iv.boot_counts
    assert counts.shape == (N_POINTS,) + tmg.results.shape and (counts.sum(-1) == SHOTS).all()
    host = _host_distances(tmg, counts, tmg.reconstructed_state, "lin")
    assert np.abs(iv.boot_dist - host).max() <= TOL[dst]
    again = qp.BootstrapStateInterval(tmg, n_points=N_POINTS, method="lin", sampler="device", seed=5)
    again.setup()
    assert np.array_equal(again.boot_counts, counts) and np.array_equal(again.boot_dist, iv.boot_dist)


def test_other_paths_keep_the_host_loop():
    """'mle-constr' and a custom callable are not the engine's: no ShardedSample, the host distances as before."""
    import quantpy_amd as qp

    tmg, _ = _measured(2, lambda a, b: qp.trace_dst(a, b), "lin")
    iv = qp.BootstrapStateInterval(tmg, n_points=3, method="lin")
    iv.setup()
    assert not hasattr(iv, "sample") and iv.boot_dist.shape == (3,)


# ---- 5. MHMCStateInterval ------------------------------------------------------------------------------------------------
def _chain(dst):
    import quantpy_amd as qp

    tmg, _ = _measured(2, dst, "mle", seed=32)
    np.random.seed(33)
    iv = qp.MHMCStateInterval(tmg, n_points=40, burn_steps=60)
    iv.setup()
    return tmg, iv


@pytest.fixture(scope="module")
def hs_chain():
    return _chain("hs")


@pytest.mark.parametrize("dst", ["trace", "if"])
def test_mhmc_interval(hs_chain, dst):
    tmg, iv = _chain(dst)
    assert iv.samples.shape == (40, 16) and np.array_equal(iv.samples, hs_chain[1].samples)
    centre = np.asarray(iv.state.matrix, dtype=np.complex128)
    mats = tmg._engine().chol_unparam(iv.samples)
    host = np.sort([tmg.dst(m, centre) for m in mats])
    print(dst, "max diff", np.abs(iv.cl_to_dist.y - host).max())
    assert iv.cl_to_dist.y.shape == (40,) and np.abs(iv.cl_to_dist.y - host).max() <= TOL[dst]
    assert np.array_equal(iv(LEVELS)[0], interp1d(np.linspace(0, 1, 40), iv.cl_to_dist.y)(LEVELS))


# ---- 6. the study --------------------------------------------------------------------------------------------------------
N_ITER, STUDY_POINTS, STUDY_SHOTS = 5, 7, 1000
# The key of the study below.  2024 is the first one tried: with 35 comparisons per case and distances spread over
# ~1e-2, one within 1e-6 of its threshold is a 1e-3 event, and the recomputation asserts that this key has none.
STUDY_SEED = 2024


@pytest.mark.parametrize("method_boot", ["lin", "mle"])
@pytest.mark.parametrize("n", [1, 2])
def test_boot_study_hs_is_the_existing_study(n, method_boot):
    from quantpy_amd import metrics

    state = _ginibre_state(n, 80 + n)
    kw = dict(n_iter=N_ITER, n_points=STUDY_POINTS, n_measurements=STUDY_SHOTS, method_boot=method_boot, seed=STUDY_SEED,
              return_details=True)
    new = metrics.get_CL_list_state_boot(state, dst="hs", **kw)
    old = metrics.get_CL_list_state(state, interval="boot", **kw)
    assert sorted(new) == sorted(old)
    for key in old:
        a, b = np.asarray(new[key]), np.asarray(old[key])
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key
    kw.pop("return_details")
    assert np.array_equal(metrics.get_CL_list_state_boot(state, **kw), np.sort(old["levels"]))  # dst='hs' is the default


@pytest.mark.parametrize("dst", ["trace", "if"])
@pytest.mark.parametrize("method_boot", ["lin", "mle"])
@pytest.mark.parametrize("n", [1, 2])
def test_boot_study_from_the_documented_keys(n, method_boot, dst):
    """Every resample redrawn from key `seed`, rows (r * n_iter + t) * S .. + S, with the ungrouped sampler, reconstructed
    with point_estimate_batch and measured on the host.  A comparison with |dist - delta_t| <= 1e-6 is left out (the engine's
    distance and the host's may fall on different sides); at most one trial may have one, and this key has none."""
    import quantpy_amd as qp
    from quantpy_amd import metrics

    state = _ginibre_state(n, 80 + n)
    host_dst = {"trace": qp.trace_dst, "if": qp.if_dst}[dst]
    kw = dict(n_iter=N_ITER, n_points=STUDY_POINTS, n_measurements=STUDY_SHOTS, method_boot=method_boot, dst=dst,
              seed=STUDY_SEED, return_details=True)
    out = metrics.get_CL_list_state_boot(state, **kw)
    assert out["seed"] == STUDY_SEED + 1 and out["counts"].shape[0] == N_ITER
    tmg = qp.StateTomograph(state)
    tmg.povm_matrix = qp.generate_measurement_matrix("proj-set", n)
    tmg.n_measurements = np.ones(tmg.povm_matrix.shape[0]) * STUDY_SHOTS
    eng = tmg._engine()
    n_set = eng.S
    rho, _ = tmg.point_estimate_batch(out["counts"], method="lin")
    assert np.array_equal(rho, out["estimates"])
    delta = np.array([host_dst(r, state.matrix) for r in rho], dtype=np.float64)
    assert np.abs(out["delta"] - delta).max() <= TOL[dst]
    pvals = np.clip(eng.born_probs(eng.bloch_from_matrix(rho)), 0, 1)
    shots = np.full(n_set, STUDY_SHOTS, dtype=np.int64)
    sure, near = np.zeros(N_ITER, dtype=np.int64), np.zeros(N_ITER, dtype=np.int64)
    for t in range(N_ITER):
        resamples = np.stack([eng.device_multinomial(shots, pvals[t], n_set, out["seed"], first_row=(r * N_ITER + t) * n_set)
                              for r in range(STUDY_POINTS)])
        est, _ = tmg.point_estimate_batch(resamples, method=method_boot)
        dist = np.array([host_dst(e, rho[t]) for e in est], dtype=np.float64)
        close = np.abs(dist - out["delta"][t]) <= 1e-6
        sure[t], near[t] = (out["delta"][t] > dist)[~close].sum(), close.sum()
        print(n, method_boot, dst, "trial", t, "delta", out["delta"][t], "dist", dist, "hits", out["hits"][t])
    assert (near > 0).sum() <= 1
    assert ((out["hits"] >= sure) & (out["hits"] <= sure + near)).all(), (out["hits"], sure, near)
    assert not near.any()  # (how STUDY_SEED was chosen)
    cls = np.linspace(0, 1, STUDY_POINTS)
    assert np.array_equal(out["levels"], [cls[h - 1] if h else 0.0 for h in out["hits"]])
    # the table does not depend on the chunking, and the plain call returns the sorted levels
    again = metrics.get_CL_list_state_boot(state, chunk=2, **kw)
    assert np.array_equal(again["hits"], out["hits"]) and np.array_equal(again["counts"], out["counts"])
    kw.pop("return_details")
    assert np.array_equal(metrics.get_CL_list_state_boot(state, chunk=1, **kw), np.sort(out["levels"]))
