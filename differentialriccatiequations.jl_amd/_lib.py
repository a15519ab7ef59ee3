"""ctypes binding of libdre_hip.so (include/dre_hip.h).  No torch types cross this boundary.

The library is built in-tree by `__graft_entry__.build()` / `make -C csrc`.  There is no CPU fallback:
if the shared object is missing the import fails loudly, and if no HIP device is usable
`dre_ctx_create` returns DRE_ERR_NODEVICE which is raised as `DREError`.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DRE_HIP_LIB") or os.path.join(_HERE, "libdre_hip.so")      # DRE_HIP_LIB: another build of the same library (A/B timing)


class DREError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libdre_hip error {code}: {msg}")
        self.code = code


class AdiOptionsC(C.Structure):
    _fields_ = [
        ("maxiters", C.c_int32),
        ("reltol", C.c_double),
        ("abstol", C.c_double),
        ("ignore_initial_guess", C.c_int32),
        ("compression_interval", C.c_int32),
        ("compression", C.c_int32),
        ("shift_kind", C.c_int32),
        ("n_history", C.c_int32),
        ("nshifts", C.c_int32),
        ("shifts_re", C.POINTER(C.c_double)),
        ("shifts_im", C.POINTER(C.c_double)),
        ("compress_tolfac", C.c_double),
        ("compress_exact", C.c_int32),
        ("heuristic_kplus", C.c_int32),
        ("heuristic_kminus", C.c_int32),
        ("inner_solve", C.c_void_p),
        ("inner_user", C.c_void_p),
        ("shift_fn", C.c_void_p),
        ("shift_user", C.c_void_p),
    ]


# dre_block_solver_fn (include/dre_hip.h): int (*)(void* user, int n, int nrhs, double cA, double cE_re, double cE_im, const double* B, double* X_re, double* X_im)
# dre_shift_fn (include/dre_hip.h): int (*)(void* user, int restart, int n, int hist_cols, const double* hist, int ldh, int capacity, double* re, double* im, int* count)
SHIFT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int))
BLOCK_SOLVER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p)


class GemmViewC(C.Structure):
    """dre_gemm_view: rows x cols, column-major with leading dimension ld, `offset` elements into the dre_dense `buf`."""
    _fields_ = [("buf", C.c_void_p), ("offset", C.c_int64), ("ld", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32)]


class GemmProductC(C.Structure):
    _fields_ = [("A", GemmViewC), ("B", GemmViewC), ("C", GemmViewC), ("copy_dst", GemmViewC), ("alpha", C.c_double)]


class GemmProbeOptionsC(C.Structure):
    _fields_ = [
        ("batch", C.c_int32),
        ("stride_a", C.c_int64), ("stride_b", C.c_int64), ("stride_c", C.c_int64),
        ("member_on", C.POINTER(C.c_int32)),
        ("coef", C.POINTER(C.c_double)), ("coef_stride", C.c_int64),
        ("rowmap", C.POINTER(C.c_int32)),
        ("cz", C.c_int64),
        ("nprod", C.c_int32), ("prod", C.POINTER(GemmProductC)),
        ("use_done", C.c_int32), ("done", C.c_int32),
        ("use_count", C.c_int32), ("iters", C.c_int32), ("base", C.c_int32), ("nmax", C.c_int32), ("per", C.c_int32),
        ("tile_sumsq", C.c_void_p),
    ]


class AdiChainProbeArgsC(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n", C.c_int32), ("m", C.c_int32), ("k", C.c_int32),
        ("nstack", C.c_int32), ("ncyc", C.c_int32), ("g", C.c_int32), ("nit", C.c_int32),
        ("base_it", C.c_int32), ("maxiters", C.c_int32), ("tdiag", C.c_int32), ("mode", C.c_int32),
        ("nt", C.c_int32), ("ld", C.c_int32),
        ("alpha", C.c_double), ("abstol", C.c_double),
        ("stacks", C.c_void_p), ("wks", C.c_void_p), ("wks_null", C.c_void_p), ("cycle", C.c_void_p), ("mu", C.c_void_p), ("R0", C.c_void_p), ("T", C.c_void_p),
        ("V", C.c_void_p), ("R", C.c_void_p), ("packs", C.c_void_p), ("Rp", C.c_void_p), ("G", C.c_void_p),
        ("state_i", C.c_void_p), ("state_d", C.c_void_p),
    ]


class WarmProbeArgsC(C.Structure):
    _fields_ = [
        ("stage", C.c_int32), ("n", C.c_int32), ("q", C.c_int32), ("m", C.c_int32),
        ("kl", C.c_int32), ("qn", C.c_int32), ("nparts", C.c_int32), ("mode", C.c_int32),
        ("ldpad", C.c_int32), ("reserved", C.c_int32),
        ("reltol", C.c_double), ("abstol", C.c_double), ("frac", C.c_double), ("budget_frac", C.c_double),
        ("Q", C.c_void_p), ("Yf", C.c_void_p), ("Pf", C.c_void_p), ("Z1", C.c_void_p), ("Cw", C.c_void_p), ("Res", C.c_void_p), ("Cc", C.c_void_p), ("parts", C.c_void_p),
        ("S", C.c_void_p), ("Wk", C.c_void_p), ("Yp", C.c_void_p), ("Pp", C.c_void_p), ("tols_in", C.c_void_p), ("basis", C.c_void_p),
        ("Z1_out", C.c_void_p), ("Cw_out", C.c_void_p), ("slab", C.c_void_p), ("Zb", C.c_void_p), ("Zy", C.c_void_p), ("W2", C.c_void_p), ("tols", C.c_void_p),
        ("Uc", C.c_void_p), ("T", C.c_void_p), ("Cp", C.c_void_p), ("Mout", C.c_void_p), ("LTout", C.c_void_p), ("U", C.c_void_p), ("R", C.c_void_p),
        ("basis_out", C.c_void_p),
        ("ticket", C.c_void_p),
    ]


_vp = C.c_void_p
_pvp = C.POINTER(C.c_void_p)
_pd = C.POINTER(C.c_double)
_pi64 = C.POINTER(C.c_int64)
_pi32 = C.POINTER(C.c_int32)
_pint = C.POINTER(C.c_int)

# name -> (restype, argtypes); every symbol declared in include/dre_hip.h appears here
PROTOTYPES = {
    "dre_version": (C.c_int, []),
    "dre_ctx_create": (C.c_int, [C.c_int, _pvp]),
    "dre_ctx_destroy": (C.c_int, [_vp]),
    "dre_last_error": (C.c_char_p, [_vp]),
    "dre_ctx_sync": (C.c_int, [_vp]),
    "dre_ctx_info": (C.c_int, [_vp, _pi64]),
    "dre_ctx_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "dre_ctx_get_option": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    "dre_prof_enable": (C.c_int, [_vp, C.c_int]),
    "dre_prof_reset": (C.c_int, [_vp]),
    "dre_prof_count": (C.c_int, [_vp, _pint]),
    "dre_prof_get": (C.c_int, [_vp, C.c_int, C.c_char_p, C.c_int, _pd, _pi64, _pd, _pd]),
    "dre_dense_upload": (C.c_int, [_vp, C.c_int, C.c_int, _pd, C.c_int, _pvp]),
    "dre_dense_create": (C.c_int, [_vp, C.c_int, C.c_int, _pvp]),
    "dre_dense_download": (C.c_int, [_vp, _vp, _pd, C.c_int]),
    "dre_dense_from_device": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _pvp]),
    "dre_dense_to_device": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "dre_dense_shape": (C.c_int, [_vp, _pint, _pint]),
    "dre_dense_free": (C.c_int, [_vp, _vp]),
    "dre_pencil_create": (C.c_int, [_vp, C.c_int, _pi64, _pi64, _pd, _pi64, _pi64, _pd, C.c_int, C.c_int, _pvp]),
    "dre_pencil_create_host": (C.c_int, [C.c_int, _pi64, _pi64, _pd, _pi64, _pi64, _pd, C.c_int, C.c_int, _pvp]),
    "dre_pencil_free": (C.c_int, [_vp]),
    "dre_pencil_info": (C.c_int, [_vp, _pi64]),
    "dre_pencil_get_array": (C.c_int, [_vp, C.c_char_p, _pi64, C.c_int64, _pi64]),
    "dre_pencil_get_values": (C.c_int, [_vp, C.c_int, _pd, C.c_int64]),
    "dre_gemm": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp, _vp, C.c_double, _vp]),
    "dre_gemm_probe": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(GemmViewC), C.POINTER(GemmViewC), C.c_double, C.POINTER(GemmViewC),
                                 C.POINTER(GemmProbeOptionsC), _pint]),
    "dre_spmm": (C.c_int, [_vp, _vp, C.c_int, C.c_double, _vp, C.c_double, _vp]),
    "dre_orthf": (C.c_int, [_vp, _vp, _pvp, _pvp]),
    "dre_sym_eig": (C.c_int, [_vp, _vp, C.c_double, _pvp, _pvp]),
    "dre_sym_eig_probe": (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_double, C.c_int, C.c_double, _pi32, C.c_int, _pi64, _pd] + [_pvp] * 7),
    "dre_adi_chain_probe": (C.c_int, [_vp, C.POINTER(AdiChainProbeArgsC)]),
    "dre_warm_probe": (C.c_int, [_vp, C.POINTER(WarmProbeArgsC)]),
    "dre_sym_eig_jacobi": (C.c_int, [_vp, _vp, C.c_double, _pvp, _pvp, _pi64]),
    "dre_shift_factor": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _pvp]),
    "dre_shift_solve": (C.c_int, [_vp, _vp, _vp, _pvp, _pvp]),
    "dre_shift_solve_smw": (C.c_int, [_vp, _vp, C.c_double, _vp, _vp, _vp, _pvp, _pvp]),
    "dre_factor_growth": (C.c_int, [_vp, _vp, _pd]),
    "dre_factor_perturbed": (C.c_int, [_vp, _vp, _pi64]),
    "dre_factor_free": (C.c_int, [_vp, _vp]),
    "dre_ldlt_create": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, _pvp]),
    "dre_ldlt_zero": (C.c_int, [_vp, _vp, C.c_int, _pvp]),
    "dre_ldlt_free": (C.c_int, [_vp, _vp]),
    "dre_ldlt_info": (C.c_int, [_vp, _pint, _pint, _pint]),
    "dre_ldlt_add": (C.c_int, [_vp, _vp, _vp, _pvp]),
    "dre_ldlt_scale": (C.c_int, [_vp, _vp, C.c_double, _pvp]),
    "dre_ldlt_concatenate": (C.c_int, [_vp, _vp]),
    "dre_ldlt_compress": (C.c_int, [_vp, _vp]),
    "dre_ldlt_compress_tol": (C.c_int, [_vp, _vp, C.c_double]),
    "dre_ldlt_norm": (C.c_int, [_vp, _vp, _pd]),
    "dre_ldlt_canonicalize": (C.c_int, [_vp, _vp]),
    "dre_ldlt_destructure": (C.c_int, [_vp, _vp, _pd, _pd, C.c_int, _pd, C.c_int]),
    "dre_adi_default_options": (C.c_int, [C.POINTER(AdiOptionsC)]),
    "dre_gale_solve": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, C.POINTER(AdiOptionsC), _pvp]),
    "dre_ldlt_dot": (C.c_int, [_vp, _vp, _vp, _pd]),
    "dre_ldlt_compress_fast": (C.c_int, [_vp, _vp]),
    "dre_gare_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp, C.c_double, _pvp]),
    "dre_ldlt_feedback": (C.c_int, [_vp, _vp, _vp, _vp, _pvp]),
    "dre_gale_apply": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _pvp]),
    "dre_adi_init": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, C.POINTER(AdiOptionsC), _pvp]),
    "dre_adi_step": (C.c_int, [_vp, _vp]),
    "dre_adi_solve": (C.c_int, [_vp, _vp]),
    "dre_adi_isdone": (C.c_int, [_vp, _pint]),
    "dre_adi_state": (C.c_int, [_vp, _pi64, _pd, _pd]),
    "dre_adi_finish": (C.c_int, [_vp, _vp, _pvp]),
    "dre_comm_unique_id": (C.c_int, [_vp, _vp]),
    "dre_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "dre_ctx_set_orthf": (C.c_int, [_vp, _vp, _vp]),
    "dre_comm_init_host": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "dre_comm_free": (C.c_int, [_vp]),
    "dre_comm_info": (C.c_int, [_vp, _pi64]),
    "dre_comm_allgather": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "dre_comm_allreduce_sum": (C.c_int, [_vp, _vp, C.c_size_t]),
    "dre_adi_snapshot": (C.c_int, [_vp, _vp, _pvp, _pvp]),
    "dre_adi_shifts": (C.c_int, [_vp, C.c_int64, _pi64, _pd, _pd]),
    "dre_adi_free": (C.c_int, [_vp]),
    "dre_heuristic_ritz": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, C.c_int, C.c_int, _pd, _pd, _pd, _pd]),
    "dre_gale_residual": (C.c_int, [_vp, _vp, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _pvp]),
    "dre_adi_result_info": (C.c_int, [_vp, _pi64, _pd]),
    "dre_adi_result_history": (C.c_int, [_vp, _pd, _pi32, _pd, _pd]),
    "dre_adi_result_take_x": (C.c_int, [_vp, _pvp]),
    "dre_adi_result_take_residual": (C.c_int, [_vp, _pvp]),
    "dre_adi_result_free": (C.c_int, [_vp]),
    "dre_gdre_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(AdiOptionsC), _pvp]),
    "dre_gdre_result_info": (C.c_int, [_vp, _pi64]),
    "dre_gdre_result_times": (C.c_int, [_vp, _pd]),
    "dre_gdre_result_K": (C.c_int, [_vp, _vp, C.c_int, _pd, C.c_int]),
    "dre_gdre_result_K_device": (C.c_int, [_vp, _vp, _vp]),
    "dre_gdre_result_K_all": (C.c_int, [_vp, _vp, _pd]),
    "dre_gdre_result_X": (C.c_int, [_vp, C.c_int, _pvp]),
    "dre_gdre_result_gale": (C.c_int, [_vp, C.c_int, _pi64, _pd]),
    "dre_gdre_result_gale_history": (C.c_int, [_vp, C.c_int, _pi64, _pd, _pi32, _pd, _pd]),
    "dre_gdre_result_gales_all": (C.c_int, [_vp, _pi64, _pd, _pd, _pi32, _pd, _pd]),
    "dre_gdre_result_free": (C.c_int, [_vp]),
    "dre_dense_gale_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd]),
    "dre_dense_invert": (C.c_int, [_vp, _vp, _pi32, _pd]),
    "dre_dense_gare_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd]),
    "dre_dense_gare_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pvp, _pd]),
    "dre_dense_gdre_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _pvp]),
    "dre_dense_gdre_solve_adaptive": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double, C.c_double,
                                                 C.c_double, C.c_int64, _pd, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, _pvp]),
    "dre_gdre_result_step_stats": (C.c_int, [_vp, _pi64, _pd]),
    "dre_gdre_result_X_dense": (C.c_int, [_vp, _vp, C.c_int, _pvp]),
    "dre_gdre_result_dense_stats": (C.c_int, [_vp, _pi64, _pi64, _pd]),
    "dre_host_eigvals": (C.c_int, [C.c_int, _pd, _pd, _pd]),
    "dre_host_gen_eigvals": (C.c_int, [C.c_int, _pd, _pd, _pd, _pd]),
    "dre_sign_create": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_double, _pvp]),
    "dre_sign_info": (C.c_int, [_vp, _pi64]),
    "dre_sign_solve_lr": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _pvp, _pvp, _pi64, _pd]),
    "dre_sign_solve_dense": (C.c_int, [_vp, _vp, _vp, C.c_int, _pvp, _pi64, _pd]),
    "dre_sign_solve_dense_t": (C.c_int, [_vp, _vp, _vp, C.c_int, _pvp, _pi64, _pd]),
    "dre_sign_solve_lr_t": (C.c_int, [_vp, _vp, _vp, _vp, C.c_double, C.c_int, C.c_int, _pvp, _pvp, _pi64, _pd]),
    "dre_svd_jacobi": (C.c_int, [_vp, _vp, C.c_double, _pvp, _pvp, _pvp, _pi64]),
    "dre_balance_lr": (C.c_int, [_vp] * 9 + [C.c_int, C.c_double] + [_pvp] * 6 + [_pi64, _pd]),
    "dre_dense_gare_solve_pair": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _pvp, _pvp, _pi64, _pd]),
    "dre_lqg_balance": (C.c_int, [_vp] * 7 + [C.c_int, C.c_double] + [_pvp] * 9 + [_pi64, _pd]),
    "dre_dense_stein_solve": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, _pvp, _pi64, _pd]),
    "dre_dense_stein_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _pvp, _pd, _pd]),
    "dre_dense_dare_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd]),
    "dre_dense_dare_solve_pair": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, _pvp, _pvp, _pi64, _pd]),
    "dre_dense_dare_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _pvp, _pd, _pd]),
    "dre_sign_free": (C.c_int, [_vp, _vp]),
    "dre_dense_sylvester_solve": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd]),
    "dre_dense_sylvester_residual": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _pvp, _pd, _pd]),
    "dre_sylvester_create": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, _pvp]),
    "dre_sylvester_solve": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _pvp, _pi64, _pd]),
    "dre_sylvester_iters": (C.c_int, [_vp, _pi64]),
    "dre_sylvester_destroy": (C.c_int, [_vp, _vp]),
    "dre_host_svd_left": (C.c_int, [C.c_int, C.c_int, _pd, _pd, _pd]),
    "dre_dense_invert_batched": (C.c_int, [_vp, C.c_int, _pvp, _pi32, _pd, _pi32]),
    "dre_dense_gale_solve_batched": (C.c_int, [_vp, C.c_int, _pvp, _pvp, _pvp, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd, _pi32]),
    "dre_dense_gdre_solve_batched": (C.c_int, [_vp, C.c_int, _pvp, _pvp, _pvp, _pvp, _pvp, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int,
                                                C.c_int, C.c_double, C.c_int, _pvp, _pi32]),
    "dre_dense_gare_solve_batched": (C.c_int, [_vp, C.c_int, _pvp, _pvp, _pvp, _pvp, _pvp, _pvp, C.c_int, C.c_double, C.c_int, _pvp, _pi64, _pd, _pi32]),
    "dre_batch_member_error": (C.c_char_p, [_vp, C.c_int]),
    "dre_sym_eig_jacobi_batched": (C.c_int, [_vp, C.c_int, _pvp, C.c_double, _pvp, _pvp, _pi64, _pi32]),
    "dre_svd_jacobi_batched": (C.c_int, [_vp, C.c_int, _pvp, C.c_double, _pvp, _pvp, _pvp, _pi64, _pi32]),
    "dre_balance_lr_batched": (C.c_int, [_vp, C.c_int] + [_pvp] * 8 + [C.c_int, C.c_double] + [_pvp] * 6 + [_pi64, _pd, _pi32]),
    "dre_freq_response": (C.c_int, [_vp] * 5 + [C.c_int, _pd, C.c_int, _pd, _pd, _pi32, _pi64]),
    "dre_freq_response_batched": (C.c_int, [_vp, C.c_int] + [_pvp] * 4 + [C.c_int, _pd, C.c_int, _pd, _pd, _pi32, _pi64]),
    "dre_dense_invert_complex_batched": (C.c_int, [_vp, C.c_int, _pvp, _pvp, _pi32, _pd, _pi32]),
    "dre_transfer_eval": (C.c_int, [_vp] * 5 + [C.c_int, _pd, _pd, C.c_int, _pd, _pd, _pi32, _pi64]),
    "dre_transfer_eval_batched": (C.c_int, [_vp, C.c_int] + [_pvp] * 4 + [C.c_int, _pd, _pd, C.c_int, _pd, _pd, _pi32, _pi64]),
    "dre_time_response": (C.c_int, [_vp] * 5 + [C.c_int, C.c_double, C.c_int, C.c_int, _pd, C.c_int, _pd, C.c_int, _pd, _pi64]),
}

_lib = None


def load():
    """Load libdre_hip.so and attach prototypes; raises if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C csrc). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx_ptr, rc):
    if rc != 0:
        msg = load().dre_last_error(ctx_ptr)
        raise DREError(rc, msg.decode() if msg else "")
    return rc
