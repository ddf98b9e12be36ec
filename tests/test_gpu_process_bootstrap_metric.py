"""GPU: the process bootstrap in trace distance -- metrics.get_CL_list_channel_boot_dst and BootstrapProcessInterval on
a tomograph whose distance is the trace distance.

The study's hits are counted again from the documented keying of the resamples (tests/test_gpu_process_bootstrap_coverage.py
does the same for the Hilbert-Schmidt distance): redraw resample r of trial t from row ((r n_iter + t) D + i) S + s of the
table of the estimates' outcome probabilities, reconstruct it with `lifp` and measure it with `metric_dist_dim` -- the
entries the study's chunks run, on other batch sizes -- so the count is pinned as long as no distance lies within 1e-13
of its delta (a condition on the inputs, asserted).

The interval is compared with the host loop it replaces, `trace_dst` on every resampled Choi matrix, within 1e-7: the
accuracy `get_CL_list_state_boot` documents for these kernels against SciPy's sqrtm."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHOTS = 1000
TOL = 1e-13


def test_study_in_trace_distance_from_the_documented_keys():
    import quantpy_amd as qp
    from quantpy_amd import metrics

    n, n_iter, n_points, seed = 1, 3, 8, 1235
    channel = qp.channel.depolarizing(0.1, n)
    kw = dict(n_iter=n_iter, n_points=n_points, n_measurements=SHOTS, seed=seed, dst="trace")
    out = metrics.get_CL_list_channel_boot_dst(channel, return_details=True, **kw)
    assert out["seed"] == seed + 1
    tmg = qp.ProcessTomograph(channel, "proj4", "hs")
    counts = tmg.experiment_batch(SHOTS, "proj-set", repeats=n_iter, sampler="device", seed=seed)
    assert np.array_equal(out["counts"], counts)
    estimates = tmg.point_estimate_batch(counts, method="lifp")
    eng = tmg._engine()
    assert np.array_equal(out["estimates"], estimates)
    assert np.array_equal(out["delta"], eng.metric_dist_dim(estimates, channel.choi.matrix, "trace"))
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
    for chunk in (1, 3):
        again = metrics.get_CL_list_channel_boot_dst(channel, return_details=True, chunk=chunk, **kw)
        assert np.array_equal(again["hits"], hits) and np.array_equal(again["counts"], counts)
    assert np.array_equal(metrics.get_CL_list_channel_boot_dst(channel, **kw), np.sort(out["levels"]))


def test_study_in_hs_is_the_study_without_a_distance():
    import quantpy_amd as qp
    from quantpy_amd import geometry, metrics

    channel = qp.channel.depolarizing(0.1, 1)
    kw = dict(n_iter=3, n_points=8, n_measurements=SHOTS, seed=1235, return_details=True)
    plain = metrics.get_CL_list_channel_boot(channel, **kw)
    for dst in ("hs", geometry.hs_dst):
        hs = metrics.get_CL_list_channel_boot_dst(channel, dst=dst, **kw)
        assert sorted(plain) == sorted(hs)
        for key in plain:
            assert np.array_equal(plain[key], hs[key]), key


def test_study_in_infidelity_is_degenerate_as_documented():
    """Choi matrices have trace 2^n: if_dst of two of them is 1 - (about 2^n)^2 < 1e-15, returned as 0."""
    import quantpy_amd as qp
    from quantpy_amd import metrics

    out = metrics.get_CL_list_channel_boot_dst(qp.channel.depolarizing(0.1, 1), n_iter=3, n_points=8,
                                               n_measurements=SHOTS, seed=1235, dst="if", return_details=True)
    assert not out["delta"].any() and not out["hits"].any() and not out["levels"].any()


@pytest.mark.parametrize("n", [1, 2])
def test_interval_in_trace_distance_against_the_host_loop(n):
    import quantpy_amd as qp
    from quantpy_amd.geometry import trace_dst
    from quantpy_amd.qobj import Qobj

    np.random.seed(11 + n)
    tmg = qp.ProcessTomograph(qp.channel.depolarizing(0.1, n), dst="trace")
    tmg.experiment(SHOTS, "proj-set")
    tmg.point_estimate("lifp")
    state = np.random.get_state()
    iv = qp.BootstrapProcessInterval(tmg, n_points=6)
    iv.setup()
    np.random.set_state(state)
    boot = qp.ProcessTomograph(tmg.reconstructed_channel, tmg.input_states, tmg.dst)
    first = tmg.tomographs[0]
    counts = boot.experiment_batch(first.n_measurements, povm=first.povm_matrix, repeats=6)
    assert np.array_equal(iv.boot_counts, counts)
    choi = boot.point_estimate_batch(counts, method="lifp", cptp=True)
    centre = tmg.reconstructed_channel.choi
    want = np.array([trace_dst(Qobj(c), centre) for c in choi], dtype=np.float64)
    err = np.abs(iv.boot_dist - want).max()
    print(f"n={n}: max |boot_dist - host loop| {err:.2e}, distances in [{want.min():.3e}, {want.max():.3e}]")
    assert iv.boot_dist.shape == (6,) and want.min() > 1e-4
    assert err < 1e-7
    eng = qp.get_engine(n)
    assert np.array_equal(iv.boot_dist, eng.metric_dist_dim(choi, centre.matrix, "trace"))
