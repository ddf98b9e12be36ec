"""GPU: the intervals and the bootstrap study of a three-qubit channel in trace distance -- 64 x 64 Choi matrices measured
by the engine (qt_metric_dist_mat, csrc/qt_metric_dim64.h) where MHMCProcessInterval and BootstrapProcessInterval looped
over `trace_dst` on the host and metrics.get_CL_list_channel_boot_dst was refused.

A depolarizing channel, 'proj-set', 1000 shots per setting, as tests/test_gpu_process3.py sets one up.  The chain and the
reconstructions are untouched: samples and resampled Choi matrices are compared bit for bit with what the
Hilbert-Schmidt runs give, the distances bit for bit with `Engine.metric_dist_dim` on the same matrices and within 1e-7
of the host loop they replace (the bound of the n = 1, 2 tests, tests/test_gpu_process_bootstrap_metric.py).  The study's
hits are counted again from the documented keying of the resamples, as that file does at n = 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHOTS = 1000
TOL = 1e-13


@pytest.fixture(scope="module")
def tmg3():
    """A three-qubit process tomograph with its 'lifp' estimate; the tests set `dst` themselves."""
    import quantpy_amd as qp

    np.random.seed(41)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, 3))
    tmg.experiment(SHOTS, "proj-set")
    tmg.point_estimate("lifp")
    return tmg


def test_mhmc_interval_in_trace_distance(tmg3):
    import quantpy_amd as qp
    from quantpy_amd.geometry import hs_dst, trace_dst

    runs = {}
    for name, dst in (("hs", hs_dst), ("trace", trace_dst)):
        tmg3.dst = dst
        np.random.seed(7)
        # (step: that of the reference's chains in tests/golden/mhmc3.npz, at which about half the proposals are accepted)
        iv = qp.MHMCProcessInterval(tmg3, n_points=8, burn_steps=4, step=1e-5, return_samples=True)
        runs[name] = iv.setup()
    tmg3.dst = hs_dst
    dist, cl, rate, mats = runs["trace"]
    # the chain is untouched by the distance, and it moves: the samples are not one matrix eight times
    assert rate == runs["hs"][2] and len(mats) == 8 and rate > 0 and len(np.unique(dist)) > 1
    assert np.array_equal(np.stack(mats), np.stack(runs["hs"][3]))
    centre = np.asarray(tmg3.reconstructed_channel.choi.matrix, dtype=np.complex128)
    want = np.sort([float(trace_dst(m, centre)) for m in mats])
    err = np.abs(dist - want).max()
    print(f"max |dist - host loop| {err:.2e}, distances in [{want.min():.3e}, {want.max():.3e}], acceptance {rate}")
    assert dist.shape == (8,) and np.all(np.diff(dist) >= 0)
    assert err < 1e-7
    eng = tmg3._engine()
    assert np.array_equal(dist, np.sort(eng.metric_dist_dim(np.stack(mats), centre, "trace")))


def test_bootstrap_interval_in_trace_distance(tmg3):
    import quantpy_amd as qp
    from quantpy_amd.geometry import hs_dst, trace_dst
    from quantpy_amd.qobj import Qobj

    tmg3.dst = trace_dst
    try:
        np.random.seed(12)
        state = np.random.get_state()
        iv = qp.BootstrapProcessInterval(tmg3, n_points=4, method="lifp")
        iv.setup()
        np.random.set_state(state)
        boot = qp.ProcessTomograph(tmg3.reconstructed_channel, tmg3.input_states, tmg3.dst)
        first = tmg3.tomographs[0]
        counts = boot.experiment_batch(first.n_measurements, povm=first.povm_matrix, repeats=4)
    finally:
        tmg3.dst = hs_dst
    assert np.array_equal(iv.boot_counts, counts)
    choi = boot.point_estimate_batch(counts, method="lifp", cptp=True)
    centre = tmg3.reconstructed_channel.choi
    want = np.array([trace_dst(Qobj(c), centre) for c in choi], dtype=np.float64)
    err = np.abs(iv.boot_dist - want).max()
    print(f"max |boot_dist - host loop| {err:.2e}, distances in [{want.min():.3e}, {want.max():.3e}]")
    assert iv.boot_dist.shape == (4,) and want.min() > 1e-4
    assert err < 1e-7
    assert np.array_equal(iv.boot_dist, qp.get_engine(3).metric_dist_dim(choi, centre.matrix, "trace"))


def test_study_in_trace_distance_from_the_documented_keys():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    n_iter, n_points, seed = 2, 3, 1235
    channel = qp.channel.depolarizing(0.1, 3)
    kw = dict(n_iter=n_iter, n_points=n_points, n_measurements=SHOTS, seed=seed)
    out = metrics.get_CL_list_channel_boot_dst(channel, return_details=True, dst="trace", **kw)
    assert out["seed"] == seed + 1
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=n_iter, sampler="device", seed=seed)
    assert np.array_equal(out["counts"], counts)
    estimates = tmg.point_estimate_batch(counts, method="lifp")
    eng = tmg._engine()
    assert np.array_equal(out["estimates"], estimates)
    assert np.array_equal(out["delta"], eng.metric_dist_dim(estimates, channel.choi.matrix, "trace"))
    assert (out["delta"] > 1e-4).all()
    dd, s, k = eng.D, eng.S, eng.K
    pvals = eng.process_born_probs(estimates)
    shots = np.tile(np.full(s, SHOTS, dtype=np.int64), dd)
    hits = np.zeros(n_iter, dtype=np.int64)
    for t in range(n_iter):
        resamples = np.stack([eng.device_multinomial(shots, pvals[t].reshape(dd * s, k), dd * s, seed + 1,
                                                     first_row=(r * n_iter + t) * dd * s).reshape(dd, s, k)
                              for r in range(n_points)])
        dist = eng.metric_dist_dim(eng.lifp(resamples, cptp=True), estimates[t], "trace")
        assert not (np.abs(out["delta"][t] - dist) <= TOL).any()  # the condition that pins the count
        hits[t] = (out["delta"][t] > dist).sum()
    print(f"hits {out['hits'].tolist()} / redrawn {hits.tolist()}, delta {out['delta'].tolist()}")
    assert np.array_equal(out["hits"], hits)
    assert np.array_equal(out["levels"], metrics.levels_from_hits(hits, n_points))
    # the infidelity of Choi matrices of trace 8 is 1 - (about 8)^2 < 1e-15: every level is 0
    degenerate = metrics.get_CL_list_channel_boot_dst(channel, return_details=True, dst="if", **kw)
    assert not degenerate["delta"].any() and not degenerate["hits"].any() and not degenerate["levels"].any()
