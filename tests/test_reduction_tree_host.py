"""CPU: a NumPy MODEL of the 64-lane reductions of quantpy_amd/csrc/qt_wave.h (gsum<64>, gmax<64>, gtrace<64>), stage by
stage -- it is not the device code, and it runs no kernel.  What it checks is the argument the kernels rest on: lane 63,
the only lane the reductions hand out, holds the same bits

  * whether the two cross-row stages (row_bcast15, row_bcast31) run with the partial row masks 0xA / 0xC over a
    zero-initialised destination (the old form) or with the full row mask and bound_ctrl (the new one), for the sum and
    for the maximum;
  * whether a trace goes through the full butterfly of gsum<64> on (lane is diagonal ? x : 0.0) or through gtrace<64>
    (one + 0.0, row_shr:9, three sums across the rows through scalar registers).

The lane source of each DPP control is the one of the "AMD Instinct MI300 / CDNA3 Instruction Set Architecture" guide,
section "Data Parallel Processing (DPP)", table DPP_CTRL (rows are 16 lanes; lane = 16 row + n):
  quad_perm [a, b, c, d]   lane 4 q + t reads lane 4 q + (a, b, c, d)[t]
  row_shr:s                lane n of a row reads lane n - s of the row; none for n < s
  row_half_mirror          lane n reads lane 7 - n of its half row (n < 8), 23 - n (n >= 8)
  row_mirror               lane n reads lane 15 - n of its row
  row_bcast15              every lane of row r reads lane 15 of row r - 1; none for row 0
  row_bcast31              every lane of rows 2, 3 reads lane 31; none for rows 0, 1
A lane without a source reads 0 when bound_ctrl is set and keeps the destination's old value otherwise; a lane whose row
is not in row_mask keeps the old value too.  The moved value is added to (or compared with) the lane's own, the lane's
own as the first operand, as in the device code."""
import numpy as np
import pytest

LANES = np.arange(64)
ROW, N = LANES // 16, LANES % 16


def _src(ctrl):
    """(source lane per lane, has a source)"""
    if isinstance(ctrl, tuple):  # quad_perm
        return LANES // 4 * 4 + np.array(ctrl)[LANES % 4], np.ones(64, bool)
    if ctrl == "row_half_mirror":
        return ROW * 16 + np.where(N < 8, 7 - N, 23 - N), np.ones(64, bool)
    if ctrl == "row_mirror":
        return ROW * 16 + 15 - N, np.ones(64, bool)
    if ctrl == "row_shr9":
        return np.where(N >= 9, LANES - 9, 0), N >= 9
    if ctrl == "row_bcast15":
        return np.where(ROW >= 1, ROW * 16 - 1, 0), ROW >= 1
    if ctrl == "row_bcast31":
        return np.full(64, 31), ROW >= 2
    raise ValueError(ctrl)


def dpp(v, ctrl, row_mask=0xF, bound_ctrl=True, old=None):
    """v_mov_b32_dpp on both halves of a double: the moved values, one per lane."""
    old = np.zeros(64) if old is None else old
    src, valid = _src(ctrl)
    enabled = ((row_mask >> ROW) & 1).astype(bool)
    moved = np.where(valid, v[src], 0.0 if bound_ctrl else old)
    return np.where(enabled, moved, old)


def vmax(a, b):
    """v_max_f64 as gmax uses it: of a NaN and a number the number; of two numbers the larger"""
    return np.fmax(a, b)


def nanmax(a, b):
    """nanmax of qt_wave.h, (b > a || b != b) ? b : a -- a NaN in b wins"""
    with np.errstate(invalid="ignore"):
        return np.where((b > a) | (b != b), b, a)


IN_ROW = [(1, 0, 3, 2), (2, 3, 0, 1), "row_half_mirror", "row_mirror"]


def reduce64(v, op, new):
    for ctrl in IN_ROW:
        v = op(v, dpp(v, ctrl))
    if new:
        v = op(v, dpp(v, "row_bcast15"))
        v = op(v, dpp(v, "row_bcast31"))
    else:  # partial row mask, no bound_ctrl, destination initialised to 0
        v = op(v, dpp(v, "row_bcast15", row_mask=0xA, bound_ctrl=False))
        v = op(v, dpp(v, "row_bcast31", row_mask=0xC, bound_ctrl=False))
    return v[63]


def gsum(v, new):
    with np.errstate(invalid="ignore", over="ignore"):
        return reduce64(np.array(v, dtype=np.float64), np.add, new)


def gmax(v, new, op=vmax):
    """gmax<64> of non-negative inputs: a NaN anywhere wins (one ballot), else the butterfly of v_max_f64.  With
    op = nanmax the butterfly alone, NaNs travelling through it."""
    v = np.array(v, dtype=np.float64)
    if op is vmax and np.isnan(v).any():
        return np.nan
    return reduce64(v, op, new)


def gtrace(x):
    """gtrace<64>: x one element per lane, lane = 8 i + j"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.where(LANES // 8 == LANES % 8, x, 0.0)
        v = v + 0.0
        v = v + dpp(v, "row_shr9")
        hi = v + v[45]  # lane 63: s3 + s2
        lo = v + v[9]   # lane 27: s1 + s0
        return (hi + lo[27])[63]


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same(a, b):
    return _bits(a) == _bits(b)


SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan]


def _inputs():
    """random doubles of mixed magnitude; then the same with +-0.0, +-inf and NaN dropped into random lanes, and each
    special in every single lane"""
    rng = np.random.default_rng(63)
    out = []
    for _ in range(40):
        out.append(rng.standard_normal(64) * 10.0 ** rng.integers(-8, 9, 64))
    for _ in range(200):
        v = rng.standard_normal(64) * 10.0 ** rng.integers(-3, 4, 64)
        k = rng.integers(1, 9)
        v[rng.choice(64, k, replace=False)] = rng.choice(SPECIALS, k)
        out.append(v)
    for s in SPECIALS:
        for lane in range(64):
            v = rng.standard_normal(64)
            v[lane] = s
            out.append(v)
        out.append(np.full(64, s))
    return out


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


def test_model_sums_what_it_should():
    """the model itself: integers sum exactly, and the tree is (r3 + r2) + (r1 + r0)"""
    v = np.arange(64, dtype=np.float64)
    assert gsum(v, False) == gsum(v, True) == 2016.0
    assert gmax(v, False) == gmax(v, True) == 63.0
    assert gtrace(v) == sum(9.0 * i for i in range(8))
    r = np.zeros(64)
    r[[0, 16, 32, 48]] = [1.0, 2.0**-53, 2.0**-53, -1.0]  # row totals r0 .. r3
    assert gsum(r, True) == (-1.0 + 2.0**-53) + (2.0**-53 + 1.0) == gsum(r, False)


def test_sum_lane63_same_bits_without_row_masks(inputs):
    for v in inputs:
        assert _same(gsum(v, False), gsum(v, True)), v


def test_max_lane63_same_bits_without_row_masks(inputs):
    for v in inputs:
        a = np.abs(v)  # every caller passes fabs(.)
        assert _same(gmax(a, False), gmax(a, True)), a
        assert _same(gmax(a, False, nanmax), gmax(a, True, nanmax)), a
    for lane in range(64):  # the largest value in any lane reaches lane 63
        a = np.full(64, 0.5)
        a[lane] = 2.0
        assert gmax(a, True) == 2.0 == gmax(a, False)


def test_trace_same_bits_as_the_full_butterfly(inputs):
    diag = LANES // 8 == LANES % 8
    for v in inputs:
        full = gsum(np.where(diag, v, 0.0), False)
        assert _same(full, gtrace(v)), (v[diag], full, gtrace(v))


def test_trace_of_negative_zeros_is_positive_zero():
    """the one place where leaving the first three stages out could show: they turn a -0.0 on the diagonal into +0.0"""
    v = np.full(64, -0.0)
    full = gsum(np.where(LANES // 8 == LANES % 8, v, 0.0), False)
    assert _bits(full) == _bits(0.0) == _bits(gtrace(v))
    for lane in range(0, 64, 9):  # and a single -0.0 beside positive zeros
        w = np.zeros(64)
        w[lane] = -0.0
        assert _bits(gtrace(w)) == _bits(0.0)
