"""Host: the two owners in quantpy_amd.sampling that need no GPU.  `check_pvals` is np.random.multinomial's condition
on a table, with its message; `shared_seed` on one rank is `resolve_seed`, down to the words it takes from np.random."""
import numpy as np
import pytest

from quantpy_amd.sampling import check_pvals, resolve_seed, shared_seed


def test_check_pvals_accepts_up_to_the_edge_and_refuses_above():
    edge = 1.0 + 1e-12
    at_edge = np.array([[0.25, 0.25, 0.5], [0.5, edge - 0.5, 0.0]])  # second row: the first K - 1 sum to the edge exactly
    assert at_edge[1, :-1].sum() == edge
    check_pvals(at_edge)
    above = at_edge.copy()
    above[1, 1] = np.nextafter(edge, 2.0) - 0.5  # ... and to the next double above it
    assert above[1, :-1].sum() == np.nextafter(edge, 2.0)
    with pytest.raises(ValueError) as err:
        check_pvals(above)
    assert str(err.value) == "sum(pvals[:-1]) > 1.0"
    with pytest.raises(ValueError) as err:
        check_pvals(np.array([[0.5, 0.5], [1.0 + 1e-9, -1e-9]]))  # a negative entry, even in the last column
    assert str(err.value) == "sum(pvals[:-1]) > 1.0"


@pytest.mark.parametrize("seed", [None, 0, 5, 2**64 - 1, 2**64 + 7, -1])
def test_shared_seed_on_one_rank_is_resolve_seed(seed):
    np.random.seed(99)
    expected = resolve_seed(seed)
    after = np.random.get_state()
    np.random.seed(99)
    assert shared_seed(seed) == expected and 0 <= expected < 2**64
    got = np.random.get_state()
    assert got[2] == after[2] and np.array_equal(got[1], after[1])


def test_a_missing_seed_takes_two_words_of_the_stream():
    np.random.seed(7)
    lo, hi = (int(w) for w in np.random.randint(0, 2**32, size=2, dtype=np.uint64))
    follows = np.random.random()
    np.random.seed(7)
    assert shared_seed(None) == lo | (hi << 32)
    assert np.random.random() == follows
    np.random.seed(7)
    before = np.random.get_state()
    shared_seed(12)  # a caller's key leaves the stream alone
    assert np.random.get_state()[2] == before[2]
