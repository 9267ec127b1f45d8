"""pamg -- MI355X-native multigrid hot path of Amin-Nadimy/P-A_multigrids.

Python host mirror over libpamg.so (HIP kernels for gfx950 behind the C-ABI in
include/pamg.h). See DESIGN.md.
"""
from ._lib import (ERROR, K_NAMES, NORM_L1, NORM_L2, NORM_L2_MASS, NORM_MAXABS, NORM_REF, RESIDUAL, RHS,  # noqa: F401
                   SOLVE_CONVERGED, SOLVE_MAXCYCLES, SOLVE_NONFINITE, SOURCE, TNEW, TNEW_NONLIN, TOLD, PamgError, lib)
from .solver import Mesh, SemiImplicitIterative, Sparse, csr_mul_array, default_params, unique_id  # noqa: F401

__all__ = ["Mesh", "SemiImplicitIterative", "default_params", "unique_id", "lib", "PamgError",
           "TNEW", "TOLD", "RHS", "RESIDUAL", "TNEW_NONLIN", "SOURCE", "ERROR", "K_NAMES", "NORM_REF", "NORM_MAXABS",
           "NORM_L2", "NORM_L1", "NORM_L2_MASS", "SOLVE_CONVERGED", "SOLVE_MAXCYCLES", "SOLVE_NONFINITE"]
