"""MI355X-native low-rank Rosenbrock/ADI engine — host-side mirror of the reference API.

Import as `import dre_amd` (the directory name carries a dot and cannot be imported directly;
`dre_amd.py` at the repo root loads this package under that name).
"""
from . import _lib
from ._lib import DREError
from .device import Context, DenseMatrix, DeviceLDLt, Factor, Pencil, default_context, set_default_context
from .api import (ADI, ADISolver, Backslash, BlockLinearProblem, BlockLinearSolver, ShermanMorrisonWoodbury, init, step_, isdone, solve_, Callbacks, DRESolution, FactoredSign, GALEProblem, GAREProblem, GDREProblem, GMRES, LDLt, LowRankUpdate, MatrixSign, Newton, ReducedModel, Ros1, Ros2, Ros3, Ros4, ScaledPencil, Shifts, SignFactorization, StepControl,
                  compress_, concatenate_, delta, dense_invert, dense_invert_batch, dense_invert_complex, dense_invert_complex_batch, solve_batch, dot, gare_residual, gare_residual_dense, lyapunov_apply, solve_gmres, heuristic_shifts, lowrank, lr_update, norm, orthf, quadratic_forcing,
                  residual, solve, solve_gale, solve_gale_dense, solve_gale_factored_sign, solve_gale_pair, solve_gare, solve_gare_dense, solve_gdre, superlinear_forcing, svd_jacobi, sym_eigh,
                  balanced_truncation, hankel_singular_values, sym_eigh_batch, svd_jacobi_batch, balanced_truncation_batch,
                  freq_response, freq_response_batch, sigma_response, bt_error, transfer_function, transfer_function_batch,
                  step_response, impulse_response, simulate,
                  LQGReducedModel, solve_gare_pair, lqg_balanced_truncation, lqg_characteristic_values, lqg_error,
                  Doubling, GDALEProblem, GDAREProblem, solve_gdale_dense, solve_gdare_dense, solve_gdare_pair, gdale_residual_dense, gdare_residual_dense,
                  GSYLEProblem, SylvesterFactorization, solve_gsyle_dense, gsyle_residual_dense, h2_norm, h2_inner, h2_error)
from .steel_profile import SIZES, initial_value, steel_profile

__all__ = [n for n in dir() if not n.startswith("_")]
