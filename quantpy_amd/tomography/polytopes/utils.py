"""`count_confidence` / `count_delta` under the reference's names (polytopes/utils.py) -- the host functions that
PolytopeStateInterval uses, not copies of them -- and `count_delta_batch`, the bisection of a whole batch of count
tables at several levels in one launch (qt_polytope_coverage)."""
import numpy as np

from ..interval import count_confidence, count_delta  # noqa: F401

__all__ = ["count_confidence", "count_delta", "count_delta_batch"]


def count_delta_batch(levels, counts, n_measurements, engine=None):
    """deltas[b][l] = count_delta(levels[l], clip(counts[b] / n_measurements[:, None], 1e-15, 1 - 1e-15),
    n_measurements) on the GPU.  counts: (B, S, K), or (B, D, S, K) for the stacked tomographs of a process with
    n_measurements (S,) repeated over them; levels: (L,).  -> (B, L) float64.  Within 2.5e-10 of the host function
    (the width of the last bisection bracket), not bit for bit: a late step can land within rounding of the level."""
    if engine is None:
        from ...engine import any_engine

        engine = any_engine()
    return engine.polytope_coverage(counts, n_measurements, np.atleast_1d(levels), return_deltas=True)
