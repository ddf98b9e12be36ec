"""GPU: the n = 3 entries that use the 64-lane reductions of qt_wave.h and are not replayed by test_gpu_mle_diet_bits.py
give the bits recorded in tests/golden/chain_diet_bits.npz.  The fixture was written once by
tests/golden/make_golden_chain_diet.py with the library of the commit before the second "instruction diet" (cross-row
reduction stages without row masks, trace reductions from the stage where two diagonal lanes meet, the Gauss-Jordan
inverse unrolled in natural pivot order, one exit of the squaring loop): every floating-point operation that reaches a
result keeps its operands and its order, so what a call writes stays equal under np.array_equal.

Five trials (B = 5: one full workgroup of four trials and a partial one), one per class of the unprojected
linear-inversion matrix: positive definite; one negative pivot, the last; one negative pivot, not the last; two negative
pivots; all counts zero, whose count-derived entries are NaN.  qt_lin_batch (with and without the physical clip),
qt_chol_param, qt_hs_dist_dim, qt_metric_dist_group_batch (both metrics, one centre and a table) and three steps of
qt_mhmc_state run on all five; the one-launch MLE (k_mle_fused_hw: the twin's unrolled inverse) at B = 5 and the split
pair (k_mle_start: the run-time pivot order and the inverse that comes with the sweep) at B = 1030 on the first three
classes."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
from make_golden_chain_diet import MLE_PICK, NAN_TRIAL, SPLIT_B, mle_counts, replay_entries, replay_mle  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("chain_diet_bits")


def _equal(a, b):
    """np.array_equal, a NaN equal to a NaN in the same place (the fixture holds the NaN trial's outputs)"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_fixture_holds_the_classes_it_is_about(gold):
    """status of the sweep on the unprojected matrices: 0 for the positive-definite trial alone; NaN in the NaN trial's
    rows and nowhere else; both MLE calls stop at iteration 0 on classes 0 - 2"""
    assert gold["counts"].shape[0] == 5 and gold["counts"][NAN_TRIAL].sum() == 0
    assert gold["entries/chol_raw/status"].tolist() == [0, 1, 1, 1, 1]
    assert gold["entries/chol_phys/status"].tolist() == [0, 0, 0, 0, 0]
    seen = False
    for k in gold.files:
        v = gold[k]
        if k.startswith("entries/") and v.dtype.kind == "f":
            rows = set(np.argwhere(np.isnan(v))[:, 0].tolist())
            assert rows <= {NAN_TRIAL}, (k, rows)
            seen |= bool(rows)
        if k.startswith("mle_"):
            assert not np.isnan(v).any(), k
    assert seen and np.isnan(gold["entries/lin_raw/rho"][NAN_TRIAL][:, 0::2]).all()  # every real part
    assert set(MLE_PICK) == {0, 1, 2}
    for tag in ("mle_hw", "mle_split"):
        assert (gold[f"{tag}/nit"] == 0).all() and (gold[f"{tag}/status"] == 0).all()
    assert os.path.getsize(os.path.join(GOLDEN, "chain_diet_bits.npz")) < 1 << 20


def test_entries_same_bits_as_recorded(gold):
    import quantpy_amd as qp
    from quantpy_amd import _capi

    got = replay_entries(qp, _capi, gold["counts"], gold["deltas"], gold["uniforms"])
    keys = {k[len("entries/"):] for k in gold.files if k.startswith("entries/")}
    assert keys == set(got), (keys, set(got))
    for k in sorted(keys):
        assert _equal(gold["entries/" + k], got[k]), (k, gold["entries/" + k], got[k])
        if got[k].dtype.kind == "f":  # only the NaN trial's own outputs may be NaN
            assert set(np.argwhere(np.isnan(got[k]))[:, 0].tolist()) <= {NAN_TRIAL}, k


@pytest.mark.parametrize("split", [False, True], ids=["one_launch_B5", "split_B1030"])
def test_mle_same_bits_as_recorded(gold, split):
    import quantpy_amd as qp
    from quantpy_amd import _capi

    tag = "mle_split" if split else "mle_hw"
    got = replay_mle(qp, _capi, mle_counts(gold["counts"], split), split)
    assert set(got) == {k[len(tag) + 1:] for k in gold.files if k.startswith(tag + "/")}
    for k, v in got.items():
        want = gold[f"{tag}/{k}"]
        assert v.shape[0] == (SPLIT_B if split else 5)
        # the split batch repeats the five trials (the generator checked that the parent's results repeat with them)
        assert np.array_equal(v, np.resize(want, v.shape)), (tag, k)
