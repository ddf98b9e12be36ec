"""The confidence polytope of Kiktenko et al., arXiv:2109.04734: the coverage study of Fig. 1 (`verification`, the
reference's `quantpy.tomography.polytopes` with the per-(trial, level) bisection and membership test on the GPU) and
the fidelity bounds of Fig. 2 (`fidelity`: the interval classes and the study over many simulated tomographs, on the
batched LP kernels)."""
from . import fidelity, utils, verification  # noqa: F401
from .fidelity import (ProcessFidelityInterval, StateFidelityInterval, StateFidelityIntervalXL, fidelity_qpt,  # noqa: F401
                       fidelity_qst, fidelity_qst_xl)
