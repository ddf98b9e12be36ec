"""The coverage study of the confidence polytope (Kiktenko et al., arXiv:2109.04734, Fig. 1): the reference's
`quantpy.tomography.polytopes` with the per-(trial, level) bisection and membership test on the GPU."""
from . import utils, verification  # noqa: F401
