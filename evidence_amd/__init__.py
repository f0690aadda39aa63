"""evidence_amd — MI355X-native RV log-likelihood engine for nested sampling.

A from-scratch replacement for ONE hot path of nicochunger/evidence: the
per-live-point Keplerian RV forward model + Gaussian log-likelihood
(evidence/rvmodel) and the unit-cube prior transform (evidence/priors.py), behind
the reference's own sampler callback signatures.  Host code is plain Python over a
ctypes C-ABI (include/rvll.h) into hand-written HIP kernels for gfx950.  There is
no CPU fallback: without librvll.so and a HIP device the constructors raise.
"""
from ._abi import (FLAG_INVALID_ORBIT, FLAG_NONCONVERGED, FLAG_WANDERED, RvllError, RvllLibraryError)
from .data import EpochTable
from .layout import ModelLayout, compile_layout
from .priors import PriorError, PriorSpec, prior_constructor
from .engine import GpuRVModel
from .nested import run_nested_ensemble
from . import shrinkage
from . import insertion
from . import merge
from . import posterior
from . import pointwise
from . import sensitivity
from . import correlated
from . import marginals                  # the module; its entry points are marginals.marginals, marginals_arrays, credible_levels
from .marginals import credible_levels, marginals_arrays
from .shrinkage import logz_error, replicates

__all__ = ["GpuRVModel", "EpochTable", "ModelLayout", "compile_layout", "PriorSpec", "PriorError",
           "prior_constructor", "RvllError", "RvllLibraryError", "FLAG_INVALID_ORBIT", "FLAG_NONCONVERGED",
           "FLAG_WANDERED", "run_nested_ensemble", "shrinkage", "replicates", "logz_error", "insertion", "merge", "posterior", "pointwise", "sensitivity", "marginals",
           "marginals_arrays", "credible_levels", "correlated"]
__version__ = "0.1.0"
