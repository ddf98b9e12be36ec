"""GPU: the MLE kernels at n <= 3 give the bits recorded in tests/golden/mle_diet_bits.npz.  The fixture was written once
by tests/golden/make_golden_mle_diet.py with the library of the commit before the first "instruction diet" of
qt_small.h (lane-constant tables in place of run-time decoding, fused reductions, shorter scalar live ranges): such a
change keeps every floating-point operation and its order, so what a launch writes stays equal under np.array_equal.
The cases (CASES of the generator, which also holds the replay of one device-pointer call): n = 3 'proj-set' through
k_mle_fused_hw, k_mle_fused and the split pair on positive-definite and clipped trials, low-shot data (psd_project, the
serial lift), the 'mixed' start (iterating evaluations), 'sic' (the generic instantiation), n = 1, 2 with partial
waves, and the one-pass distance."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
from make_golden_mle_diet import CASES, DIST_CASE, replay  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load_golden("mle_diet_bits")


def _check(gold, prefix, got):
    keys = {k[len(prefix):] for k in gold.files if k.startswith(prefix)}
    assert keys == set(got), (prefix, keys, set(got))
    for k in sorted(keys):
        assert np.array_equal(gold[prefix + k], got[k]), (prefix + k, gold[prefix + k], got[k])


def test_fixture_holds_the_classes_it_is_about(gold):
    """Stop-at-0 trials of both kinds, iterating trials, and the twin-wave kernel where it is the default."""
    assert set(k.split("/")[0] for k in gold.files) == set(CASES) | {"dist", "dist_centre"}
    assert (gold["n3_ginibre/hw/nit"] == 0).all() and gold["n3_ginibre/hw/took_hw"]
    assert (gold["n3_rank1_lowshot/hw/nit"] > 0).all() and (gold["n3_mixed_start/fused/nit"] > 0).all()
    assert gold["n3_sic/hw/took_hw"] and gold["n3_pivot0/hw/took_hw"]
    assert os.path.getsize(os.path.join(GOLDEN, "mle_diet_bits.npz")) < 1 << 20


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_bits_as_recorded(gold, case):
    import quantpy_amd as qp
    from quantpy_amd import _capi

    for variant in CASES[case][6]:
        _check(gold, f"{case}/{variant}/", replay(qp, _capi, case, gold[f"{case}/counts"], variant))


def test_distance_epilogue_same_bits(gold):
    import quantpy_amd as qp
    from quantpy_amd import _capi

    for variant in CASES[DIST_CASE][6]:
        got = replay(qp, _capi, DIST_CASE, gold[f"{DIST_CASE}/counts"], variant, dist_centre=gold["dist_centre"])
        _check(gold, f"dist/{variant}/", got)
