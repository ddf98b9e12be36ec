"""Host: a NumPy model of the two butterflies in the specialised load_freq at n = 3 (csrc/qt_small.h): the per-setting
sums of a trial's counts over aligned groups of eight lanes and their total across the wavefront, once on doubles
(segsum_c<8>, gsum_above<8>) and once on 32-bit integers converted at the end (segsum_u32<8>, gsum_above_u32<8>: the
integer front, taken where every count of the wavefront is below 2^22).  The kernel relies on the two giving the same
float64 bit patterns; here that is checked on random counts, lane by lane, through the DPP controls the kernel uses."""
import numpy as np

M, G = 216, 64
LANES = np.arange(G)


def _quad_perm(v, perm):
    return v[(LANES & ~3) | np.asarray(perm)[LANES & 3]]


def _row_half_mirror(v):
    return v[(LANES & ~7) | (7 - (LANES & 7))]


def _row_mirror(v):
    return v[(LANES & ~15) | (15 - (LANES & 15))]


def _row_bcast(v, last):
    """row_bcast15 / row_bcast31 with a full row mask and bound_ctrl: lane 15 of a row into the next row (15), lane 31
    into rows 2 and 3 (31); a lane without a source reads 0."""
    out = np.zeros_like(v)
    if last == 15:
        for row in (1, 2, 3):
            out[16 * row:16 * row + 16] = v[16 * row - 1]
    else:
        out[32:] = v[31]
    return out


def _segsum8(v):
    v = v + _quad_perm(v, [1, 0, 3, 2])
    v = v + _quad_perm(v, [2, 3, 0, 1])
    return v + _row_half_mirror(v)


def _gsum_above8(v):
    v = v + _row_mirror(v)
    v = v + _row_bcast(v, 15)
    v = v + _row_bcast(v, 31)
    return v[63]


def _front(counts, dtype):
    """counts [216] -> (dv [4][64], st [4][64], total) as float64, the sums formed in `dtype`"""
    rows = LANES[None, :] + G * np.arange(4)[:, None]
    valid = rows < M
    v = np.where(valid, counts[np.minimum(rows, M - 1)], 0).astype(dtype)
    st = np.stack([_segsum8(v[q]) for q in range(4)])
    total = _gsum_above8((st[0] + st[1]) + (st[2] + st[3]))
    return v.astype(np.float64), st.astype(np.float64), np.float64(total)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def test_model_sums_what_it_should():
    counts = np.arange(1, M + 1, dtype=np.int64)
    dv, st, total = _front(counts, np.float64)
    assert total == counts.sum()
    assert st[0][0] == counts[:8].sum() and st[3][23] == counts[208:216].sum() and st[3][24] == 0.0


def test_integer_and_double_butterflies_same_bits():
    rng = np.random.default_rng(22)
    for trial in range(200):
        top = [1 << 22, 1 << 22, 1 << 10, 2][trial % 4]
        counts = rng.integers(0, top, size=M, dtype=np.int64)
        if trial % 4 == 0:
            counts[rng.integers(0, M)] = (1 << 22) - 1
        if trial == 1:
            counts[:] = (1 << 22) - 1  # the largest total of the fast path: 216 (2^22 - 1) < 2^30
        as_double, as_int = _front(counts, np.float64), _front(counts, np.uint32)
        assert as_int[2] == counts.sum() < 1 << 30
        for a, b in zip(as_double, as_int):
            assert np.array_equal(_bits(a), _bits(b)), trial
