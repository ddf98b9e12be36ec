"""GPU: `sampling.device_chunks`, the one chunked draw behind the bootstraps and the studies.  A table of 3 settings x 2
outcomes (period 3) and 7 units of 3 rows: whatever the chunk size and the range, the chunks concatenate to exactly those
rows of ONE unchunked `Engine.device_multinomial` with the same key -- rows are keyed by their index in the table -- and an
empty range makes no call at all."""
import numpy as np
import pytest
import torch

from quantpy_amd.engine import any_engine
from quantpy_amd.sampling import device_chunks

pytestmark = pytest.mark.gpu

SHOTS = np.array([1000, 37, 250])
PVALS = np.array([[0.5, 0.5], [0.125, 0.875], [1.0, 0.0]])
ROWS, UNITS, KEY = 3, 7, 0x9E3779B97F4A7C15


class Counting:
    """The engine, with its `device_multinomial` calls written down as (rows, first_row)."""

    def __init__(self, engine):
        self.engine, self.device, self.calls = engine, engine.device, []

    def device_multinomial(self, n, pvals, rows, seed, first_row=0, out=None):
        self.calls.append((rows, first_row))
        return self.engine.device_multinomial(n, pvals, rows, seed, first_row=first_row, out=out)


@pytest.fixture(scope="module")
def table():
    """The whole table from one call, on the host: (UNITS * ROWS, 2)."""
    full = any_engine().device_multinomial(SHOTS, PVALS, UNITS * ROWS, KEY)
    assert full.shape == (UNITS * ROWS, 2) and np.array_equal(full.sum(1), np.tile(SHOTS, UNITS))
    assert len({row.tobytes() for row in full[0::ROWS]}) > 1  # (the units differ: a wrong first_row would show)
    return full


@pytest.mark.parametrize("first,last", [(0, 7), (2, 5)])
@pytest.mark.parametrize("chunk", [1, 3, 7, 100])
def test_chunks_are_the_rows_of_the_unchunked_table(table, chunk, first, last):
    engine = Counting(any_engine())
    starts, parts = [], []
    for unit0, counts in device_chunks(engine, SHOTS, PVALS, ROWS, first, last, chunk, KEY, (ROWS, 2)):
        assert counts.is_cuda and counts.dtype == torch.int64 and counts.shape[1:] == (ROWS, 2)
        starts.append(unit0)
        parts.append(counts.cpu().numpy())  # (copied: the next chunk overwrites the buffer)
    step = min(chunk, last - first)
    assert starts == list(range(first, last, step))
    assert [p.shape[0] for p in parts] == [min(step, last - u) for u in starts]
    assert engine.calls == [(p.shape[0] * ROWS, u * ROWS) for u, p in zip(starts, parts)]
    got = np.concatenate(parts).reshape(-1, 2)
    assert got.dtype == np.int64 and got.tobytes() == table[first * ROWS: last * ROWS].tobytes()


@pytest.mark.parametrize("first,last", [(0, 0), (4, 4), (5, 2)])
def test_an_empty_range_yields_and_launches_nothing(first, last):
    engine = Counting(any_engine())
    assert list(device_chunks(engine, SHOTS, PVALS, ROWS, first, last, 3, KEY, (ROWS, 2))) == []
    assert engine.calls == []
