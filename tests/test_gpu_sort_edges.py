"""GPU: the order-statistics kernels of the bootstrap interval (interval.py:610-612) -- qt_sort_f64 (bitonic up to 8192
values, radix sort above), qt_sorted_quantiles, the four qt_select_* steps and qt_merge_sorted -- at signed zeros, NaNs of
both signs and any payload, infinities, subnormals, DBL_MAX, all-NaN / all-zero samples and massive ties, on both sides of
the 8192 switch and of k_sort_small's block-size branches.  Expected values are plain NumPy: np.sort and
interp1d(np.linspace(0, 1, n), np.sort(x)) (samples and levels: tests/test_sort_edges_host.py)."""
import numpy as np
import pytest

from test_gpu_selection import simulated_rank_quantiles
from test_sharded_quantiles import reference_quantiles
from test_sort_edges_host import KINDS, SIZES, assert_sorted_like_numpy, edge_levels, edge_sample, few_levels

pytestmark = pytest.mark.gpu

CANONICAL_NAN = 0x7FF8000000000000


@pytest.fixture(scope="module")
def eng():
    import quantpy_amd

    return quantpy_amd.get_engine(1)


def assert_canonical(srt):
    """qt_sort_f64 writes either zero as +0.0 and every NaN as 0x7ff8000000000000."""
    bits = srt.view(np.uint64)
    assert not ((srt == 0) & np.signbit(srt)).any()
    assert (bits[np.isnan(srt)] == np.uint64(CANONICAL_NAN)).all()


@pytest.mark.parametrize("kind", KINDS)
def test_sort_and_quantiles_equal_numpy(eng, kind):
    """qt_sort_f64 through host and device pointers equals np.sort by value (NaNs counted, all last, same non-NaN
    multiset) with canonical bits; qt_sorted_quantiles on it -- and on np.sort's own output, zeros interleaved and NaN signs
    as they came -- equals interp1d at 0, 1, the grid points, their nextafter neighbours and the cells next to +-inf and
    NaN, where numpy.interp's slope is inf or NaN and it retries from the other end."""
    import torch

    for n in SIZES:
        x = edge_sample(kind, n)
        want_srt = np.sort(x)
        levels = edge_levels(want_srt, n_max=4097)
        want = reference_quantiles(x, levels)
        srt, got = eng.sort_quantiles(x, levels)                      # host pointers
        assert_sorted_like_numpy(srt, x)
        assert_canonical(srt)
        assert np.array_equal(got, want, equal_nan=True), (kind, n, levels[~((got == want) | (np.isnan(got) & np.isnan(want)))])
        # device pointers, inside a larger buffer at an odd offset: the sort touches exactly its n values
        buf = torch.full((n + 2,), -7.0, dtype=torch.float64, device="cuda")
        buf[1: n + 1] = torch.from_numpy(x).cuda()
        view = buf[1: n + 1]
        eng.sort_dev(view)
        eng.sync()
        got_dev = buf.cpu().numpy()
        assert got_dev[0] == -7.0 and got_dev[-1] == -7.0, (kind, n)
        assert np.array_equal(got_dev[1: n + 1].view(np.uint64), srt.view(np.uint64)), (kind, n)
        d = torch.from_numpy(x).cuda()
        assert np.array_equal(eng.sort_quantiles(d, levels), want, equal_nan=True), (kind, n)
        assert np.array_equal(d.cpu().numpy().view(np.uint64), srt.view(np.uint64))
        raw = eng.quantiles_of_sorted(torch.from_numpy(want_srt).cuda(), levels)
        assert np.array_equal(raw, want, equal_nan=True), (kind, n)


@pytest.mark.parametrize("n", [6, 64, 8192, 8193, 2**20 + 3])
def test_sort_orders_every_nan_last_and_joins_the_zeros(eng, n):
    """The two flaws of a plain bit-flip key on both sides of the 8192 switch (bitonic / radix): 0/0's NaN (sign bit set)
    and the all-ones NaN must not sort first, and -0.0 / +0.0 must come out as one run of +0.0."""
    from test_sort_edges_host import NAN_NEG, NAN_PAYLOADS, NZERO

    x = np.full(n, 0.5)
    x[:6] = [0.3, NAN_NEG, NZERO, 0.1, 0.0, NAN_PAYLOADS[1]]
    srt, q = eng.sort_quantiles(x, np.array([0.0, 1.0]))
    assert np.isnan(srt[-2:]).all() and not np.isnan(srt[:-2]).any(), (n, srt[:3], srt[-3:])
    assert q[0] == 0.0 and np.isnan(q[1]), (n, q)
    assert srt[0] == 0.0 and srt[1] == 0.0 and not np.signbit(srt[:2]).any(), (n, srt[:4])


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 8])
def test_selection_kernels_on_edge_samples(eng, n_ranks):
    """The four qt_select_* steps with the ranks simulated on one GPU (n < ranks included): without the overflow flag the
    result is interp1d's bit for bit (as values); with it, the gather path ShardedSample takes -- qt_merge_sorted of the
    sorted shards, then qt_sorted_quantiles -- must give it.  Plus ShardedSample on a device shard at world size 1."""
    import torch

    from quantpy_amd import distributed as qd

    rng = np.random.default_rng(n_ranks)
    selected = 0
    for kind in KINDS:
        for n in SIZES:
            x = edge_sample(kind, n, seed=n_ranks)
            levels = few_levels(np.sort(x), rng)
            want = reference_quantiles(x, levels)
            plan = qd.selection_plan(n, n_ranks, len(levels))
            if plan is None:
                n_max = -(-n // n_ranks)
                stride = max(1, n_max // 16)
                plan = (stride, -(-n_max // stride), min((2 * n_ranks + 3) * stride, n_max))
            got, flag, shards = simulated_rank_quantiles(eng, x, levels, n_ranks, plan)
            if flag == 0:
                selected += 1
                assert np.array_equal(got, want, equal_nan=True), (kind, n, n_ranks, plan, got, want)
            merged = eng.merge_sorted(torch.cat(shards), [s.numel() for s in shards])
            assert_sorted_like_numpy(merged.cpu().numpy(), x)
            assert np.array_equal(eng.quantiles_of_sorted(merged, levels), want, equal_nan=True), (kind, n, n_ranks)
            if n_ranks == 1 and n > 1:
                smp = qd.ShardedSample(torch.from_numpy(x).cuda(), n, engine=eng)
                assert np.array_equal(smp.quantiles(levels), want, equal_nan=True) and smp.last_path == "local"
    assert selected > len(KINDS) * len(SIZES) // 3, selected


@pytest.mark.parametrize("ptr", ["host", "device"])
def test_merge_sorted_runs_sorted_by_numpy(eng, ptr):
    """qt_merge_sorted, R = 1 ... 9 runs, empty runs included, each run sorted by np.sort (zeros interleaved, NaNs of both
    signs last): the result is np.sort of the union by value and keeps the input bits (a permutation of them)."""
    import torch

    rng = np.random.default_rng(4)
    for kind in KINDS:
        for R in range(1, 10):
            lengths = rng.choice([0, 1, 2, 63, 64, 65, 1025, 8193], size=R)
            if R > 2:
                lengths[rng.integers(0, R)] = 0
            if kind == "everything" and R == 9:
                lengths[0] = 2**20 + 3
            x = edge_sample(kind, int(lengths.sum()) or 1, seed=R)[: int(lengths.sum())]
            at = np.concatenate([[0], np.cumsum(lengths)])
            runs = np.concatenate([np.sort(x[at[r]: at[r + 1]]) for r in range(R)])
            if ptr == "host":
                got = eng.merge_sorted(runs, lengths)
            else:
                got = eng.merge_sorted(torch.from_numpy(runs).cuda(), lengths) if len(runs) else None
                if got is None:
                    continue
                eng.sync()
                got = got.cpu().numpy()
            assert_sorted_like_numpy(got, x)
            assert np.array_equal(np.sort(got.view(np.uint64)), np.sort(runs.view(np.uint64))), (kind, R, lengths)
