"""The order-statistics path of the bootstrap interval (interval.py:610-612) at the values where a bit-flip sort key goes
wrong: signed zeros, NaNs of both signs and any payload, infinities, subnormals, DBL_MAX, all-NaN / all-zero samples and
massive ties -- CPU side: distributed.py's `_sort_keys` and the NumPy restatement of the four selection steps
(`host_splitters`, `host_bracket`, `host_window`, `host_finish`) on simulated ranks, and `ShardedSample` on a NumPy
shard.  The expected value is always plain NumPy: np.sort and interp1d(np.linspace(0, 1, n), np.sort(x)).
tests/test_gpu_sort_edges.py runs the HIP kernels on the same samples."""
import numpy as np
import pytest

from test_sharded_quantiles import reference_quantiles, simulate_ranks_host


def from_bits(*bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


# every special value by its bit pattern, so that the sign of each NaN is known
NZERO, PZERO = from_bits(0x8000000000000000, 0)
PINF, NINF = from_bits(0x7FF0000000000000, 0xFFF0000000000000)
NAN_POS = from_bits(0x7FF8000000000000)[0]        # np.nan
NAN_NEG = from_bits(0xFFF8000000000000)[0]        # what 0/0 and inf - inf give on x86
NAN_PAYLOADS = from_bits(0x7FFFFFFFFFFFFFFF,      # the splitter padding's pattern
                         0xFFFFFFFFFFFFFFFF,      # key 0 under the old bit flip: the "none" sentinel at the low end
                         0x7FF0000000000001)      # signalling NaN, lowest payload
NANS = np.concatenate([[NAN_POS, NAN_NEG], NAN_PAYLOADS])
EXTREMES = from_bits(0x1, 0x8000000000000001,                     # +-5e-324
                     0x0010000000000000, 0x8010000000000000,      # +-2.2250738585072014e-308
                     0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF)      # +-DBL_MAX

KINDS = ("zeros", "inf", "nan", "nan_payload", "extremes", "everything", "all_nan", "all_zero", "ties")
SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 20001, 2**20 + 3)


def _sprinkle(rng, x, values, frac):
    """Set a fraction `frac` (at least one slot) of x to values drawn from `values`."""
    m = max(1, int(frac * len(x)))
    at = rng.choice(len(x), size=min(m, len(x)), replace=False)
    x[at] = values[rng.integers(0, len(values), len(at))]
    return x


def edge_sample(kind, n, seed=0):
    """n float64 values of a mix: finite data of both signs plus the special values of `kind`."""
    rng = np.random.default_rng([seed, n, KINDS.index(kind)])
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
    zeros = np.array([PZERO, NZERO])
    if kind == "zeros":
        _sprinkle(rng, x, zeros, 0.3)
    elif kind == "inf":
        _sprinkle(rng, x, np.array([PINF, NINF]), 0.05)
    elif kind == "nan":
        _sprinkle(rng, x, np.array([NAN_POS, NAN_NEG]), 0.05)
    elif kind == "nan_payload":
        _sprinkle(rng, x, NAN_PAYLOADS, 0.05)
    elif kind == "extremes":
        _sprinkle(rng, x, EXTREMES, 0.1)
    elif kind == "everything":
        _sprinkle(rng, x, np.concatenate([zeros, [PINF, NINF], NANS, EXTREMES]), 0.3)
    elif kind == "all_nan":
        x = NANS[rng.integers(0, len(NANS), n)]
    elif kind == "all_zero":
        x = zeros[rng.integers(0, 2, n)]
    elif kind == "ties":  # a handful of distinct values, -0.0 among them (np.round of a small negative)
        x = np.round(rng.standard_normal(n), 1)
    return np.ascontiguousarray(x, dtype=np.float64)


def edge_levels(srt, n_max=None):
    """Levels 0 and 1, the grid points and their nextafter neighbours (all of them up to n_max points, else a stride),
    and the grid points -- with neighbours -- around every place where the sorted sample changes class (-inf, finite,
    +inf, NaN, and the zeros): the cells whose ends touch an infinity or a NaN."""
    n = len(srt)
    grid = np.linspace(0, 1, n) if n > 1 else np.array([0.0])
    pts = grid if n_max is None or n <= n_max else grid[:: -(-n // n_max)]
    cls = np.select([np.isnan(srt), srt == np.inf, srt == -np.inf, srt == 0], [3, 2, -2, 0], 1)
    edges = np.flatnonzero(np.diff(cls)) if n > 1 else np.empty(0, dtype=np.int64)
    at = np.clip(np.concatenate([edges + d for d in (-1, 0, 1, 2)]), 0, n - 1)
    pts = np.concatenate([pts, grid[at]])
    lv = np.concatenate([pts, np.nextafter(pts, 2.0), np.nextafter(pts, -1.0), [0.0, 1.0, 0.5]])
    return np.unique(np.clip(lv, 0.0, 1.0))


def few_levels(srt, rng, k=40):
    """At most 64 levels (the selection's limit): the edge levels, thinned at random, plus 0, 1 and a few random ones."""
    lv = edge_levels(srt, n_max=16)
    if len(lv) > k:
        lv = rng.choice(lv, k, replace=False)
    return np.concatenate([lv, [0.0, 1.0], rng.random(4)])


def assert_sorted_like_numpy(got, x):
    """got holds np.sort(x) by value: equal under equal_nan, the same number of NaNs, all of them last, and the same
    multiset of non-NaN values (the zeros counted together)."""
    want = np.sort(x)
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    nn = int(np.isnan(x).sum())
    assert int(np.isnan(got).sum()) == nn and (nn == 0 or np.isnan(got[len(got) - nn:]).all())
    assert np.array_equal(np.sort(got[~np.isnan(got)]), want[: len(want) - nn])


def test_sample_builders_carry_the_special_values():
    assert np.signbit(NAN_NEG) and np.isnan(NAN_NEG) and not np.signbit(NAN_POS)
    with np.errstate(invalid="ignore"):  # the NaN NumPy arithmetic makes here has the sign bit set
        made = np.array([0.0]) / np.array([0.0])
    assert np.isnan(made[0])
    x = edge_sample("everything", 20001)
    b = set(x.view(np.uint64).tolist())
    for v in np.concatenate([[NZERO, PZERO, PINF, NINF], NANS, EXTREMES]):
        assert int(np.array([v]).view(np.uint64)[0]) in b
    t = edge_sample("ties", 20001)
    assert (np.signbit(t) & (t == 0)).any() and ((~np.signbit(t)) & (t == 0)).any()


def test_sort_keys_order_like_np_sort():
    """_sort_keys is the order of np.sort: -0.0 and +0.0 share a key, every NaN (either sign, any payload) shares one key
    above +inf's, and no value has a sentinel key (0 = "none" below, ~0 = "none" above / splitter padding)."""
    from quantpy_amd.distributed import _KEY_NONE_HI, _KEY_NONE_LO, _sort_keys

    k = _sort_keys(np.array([NZERO, PZERO]))
    assert k[0] == k[1]
    kn = _sort_keys(NANS)
    assert (kn == kn[0]).all()
    assert kn[0] > _sort_keys(np.array([PINF]))[0] and kn[0] < _KEY_NONE_HI
    ordered = np.concatenate([[NINF], -EXTREMES[4:5], [-1.0], -EXTREMES[2:3], -EXTREMES[0:1], [0.0],
                              EXTREMES[0:1], EXTREMES[2:3], [1.0], EXTREMES[4:5], [PINF]])
    ko = _sort_keys(ordered)
    assert (ko[1:] > ko[:-1]).all()
    for kind in KINDS:
        x = edge_sample(kind, 4097)
        keys = _sort_keys(x)
        assert ((keys != _KEY_NONE_LO) & (keys != _KEY_NONE_HI)).all(), kind
        # np.sort's order (stable argsort by key = np.sort by value)
        assert_sorted_like_numpy(x[np.argsort(keys, kind="stable")], x)
        # a shard sorted by np.sort is monotone in the keys whatever np.sort did with the zeros and the NaNs
        ks = _sort_keys(np.sort(x))
        assert (ks[1:] >= ks[:-1]).all(), kind


@pytest.mark.parametrize("kind", KINDS)
def test_host_selection_on_simulated_ranks(kind):
    """The NumPy restatement of the four selection steps, 1, 2, 3 and 8 simulated ranks (n < ranks included), the product's
    plan and a forced one: a result is np.sort + interp1d's by value; a decline (None) needs a really clipped window."""
    from quantpy_amd import distributed as qd

    rng = np.random.default_rng(KINDS.index(kind))
    for n in SIZES:
        x = edge_sample(kind, n)
        levels = few_levels(np.sort(x), rng)
        want = reference_quantiles(x, levels)
        for n_ranks in (1, 2, 3, 8):
            plans = [qd.selection_plan(n, n_ranks, len(levels))]
            n_max = -(-n // n_ranks)
            stride = max(1, n_max // 16)
            plans.append((stride, -(-n_max // stride), min((2 * n_ranks + 3) * stride, n_max)))
            for plan in plans:
                if plan is None:
                    continue
                got, (lo, hi, all_win) = simulate_ranks_host(x, levels, n_ranks, plan)
                if got is None:
                    assert (all_win[:, :, 1] > plan[2]).any(), (kind, n, n_ranks, plan)
                    continue
                assert np.array_equal(got, want, equal_nan=True), (kind, n, n_ranks, plan, got, want)


def test_signed_zero_ties_reach_the_right_order_statistic():
    """The sample of the open finding: np.round(standard_normal(n), 1) over 2-5 ranks.  np.sort leaves -0.0 and +0.0
    interleaved in a shard; the binary searches of host_bracket / host_window must still see one run of zeros (the old
    keys made the bracket empty and host_finish raise IndexError)."""
    from quantpy_amd import distributed as qd

    rng = np.random.default_rng(11)
    declined = 0
    for case in range(120):
        n = int(rng.integers(2000, 20001))
        n_ranks = int(rng.integers(2, 6))
        x = np.round(rng.standard_normal(n), 1)
        levels = np.concatenate([rng.random(3), [0.5, 0.46, 0.54]])
        n_max = -(-n // n_ranks)
        stride = int(rng.integers(1, max(2, n_max // 8)))
        plan = (stride, -(-n_max // stride), int(rng.integers(max(1, stride), 3 * n_max + 2)))
        got, (lo, hi, all_win) = simulate_ranks_host(x, levels, n_ranks, plan)
        if got is None:
            declined += 1
            assert (all_win[:, :, 1] > plan[2]).any()
            continue
        assert np.array_equal(got, reference_quantiles(x, levels)), (case, n, n_ranks, plan)
    assert declined < 100


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_sample_numpy_world_one(kind):
    """ShardedSample on a NumPy shard at world size 1: the whole sorted sample and interp1d at every grid point, its
    neighbours and the cells next to the infinities and NaNs."""
    from quantpy_amd.distributed import ShardedSample

    for n in SIZES[:-1]:
        x = edge_sample(kind, n)
        smp = ShardedSample(x.copy(), n)
        assert_sorted_like_numpy(smp.gather_sorted(), x)
        levels = edge_levels(np.sort(x), n_max=4097)
        got = smp.quantiles(levels)
        assert smp.last_path == "local"
        assert np.array_equal(got, reference_quantiles(x, levels), equal_nan=True), (kind, n)
