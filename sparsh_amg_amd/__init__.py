"""sparsh_amg_amd -- MI355X-native AMG solve phase behind the SParSH-AMG API.

This package is a thin ctypes binding of ``libsparsh_amg.so`` (HIP kernels for gfx950 + host
setup + C ABI, sources in ``csrc/``; C ABI in ``include/sparsh_amg.h``).  There is no Python or
CPU compute path: if the native library is missing, importing fails loudly, and if no GPU is
visible every solver call raises.

Python names mirror the reference's C++ entry points (include/AMG.hpp:40-85 of
cmgcds/SParSH-AMG): ``AMG_Solver_CPU_GPU_MI(A, b, x)``, ``Solver_PCG_4(A, b, x)`` ...
where ``A`` is an :class:`sp_matrix_mg`, and ``b``/``x`` are float64 numpy vectors (``x`` is
the initial guess on entry and is overwritten with the solution, as in the reference).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import problems  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparsh_amg.so")

SPARSH_AMG, SPARSH_CG, SPARSH_PCG, SPARSH_BICG, SPARSH_PBICG = 0, 1, 2, 3, 4
SPARSH_GMRES, SPARSH_PGMRES = 5, 6
SPARSH_FCG = 7
METHODS = {"amg": SPARSH_AMG, "cg": SPARSH_CG, "pcg": SPARSH_PCG, "bicg": SPARSH_BICG, "pbicg": SPARSH_PBICG,
           "gmres": SPARSH_GMRES, "pgmres": SPARSH_PGMRES}
SPARSH_BCG = 8
BLOCK_METHODS = {"bcg": SPARSH_BCG}  # methods of solve_multi only: the columns of a block share one search space
SPARSH_MBICG = 10
# block BiCGStab, a method of solve_multi only as well; the columns are frozen one by one as in "pcg" (BLOCK_METHODS holds the
# coupled methods, whose columns share one search space)
UNSYMMETRIC_BLOCK_METHODS = {"mbicg": SPARSH_MBICG}
SPARSH_MBICG_SCALARS, SPARSH_MBICG_PARTIALS = 9, 2048
MBICG_SLOTS = ("ALPHA1", "APR0", "ALPHA", "ASS", "ASAS", "OMEGA1", "BETA", "RR0", "RES")
MBICG_FIN = {"init": 0, "alpha": 1, "omega": 2, "beta_res": 3}
FLEXIBLE_METHODS = {"fcg": SPARSH_FCG}  # methods whose preconditioner may change between applications (the K-cycle)
SPARSH_CYCLE_V, SPARSH_CYCLE_W, SPARSH_CYCLE_K = 0, 1, 2
CYCLES = {"v": SPARSH_CYCLE_V, "w": SPARSH_CYCLE_W, "k": SPARSH_CYCLE_K}
SPARSH_NULLSPACE_NONE, SPARSH_NULLSPACE_CONSTANT = 0, 1
NULLSPACES = {"none": SPARSH_NULLSPACE_NONE, "constant": SPARSH_NULLSPACE_CONSTANT}
SPARSH_SMOOTH_JACOBI, SPARSH_SMOOTH_SOR, SPARSH_SMOOTH_CHEBYSHEV = 0, 1, 3
SPARSH_SOR_FORWARD, SPARSH_SOR_SYMMETRIC = 0, 1
SPARSH_BASIS_FP64, SPARSH_BASIS_FP32 = 0, 1
GMRES_BASES = {"fp64": SPARSH_BASIS_FP64, "fp32": SPARSH_BASIS_FP32}
SMOOTHERS = {"jacobi": SPARSH_SMOOTH_JACOBI, "sor": SPARSH_SMOOTH_SOR, "chebyshev": SPARSH_SMOOTH_CHEBYSHEV}
SOR_ORDERS = {"forward": SPARSH_SOR_FORWARD, "symmetric": SPARSH_SOR_SYMMETRIC}
SPARSH_OK, SPARSH_EINVAL, SPARSH_ENODEV, SPARSH_ESTATE, SPARSH_ENUMERIC, SPARSH_ENOCONV, SPARSH_ECOMM = 0, -1, -2, -3, -4, -5, -6
SPARSH_EIG_BASIS_PLAIN, SPARSH_EIG_BASIS_ORTHO = 0, 1
SPARSH_MAX_RHS = 8



# every method name: the single-vector methods, the flexible one, and the two kinds of solve_multi only
_METHOD_CODES = {**METHODS, **FLEXIBLE_METHODS, **BLOCK_METHODS, **UNSYMMETRIC_BLOCK_METHODS}


def _method(method):
    """method code of a name ("pcg", "fcg", "mbicg", ...) or the code itself"""
    return _METHOD_CODES[method] if isinstance(method, str) else method


def multi_width(nrhs):
    """width of the interleaved device block behind nrhs columns: 2, 4 or 8"""
    return 2 if nrhs <= 2 else (4 if nrhs <= 4 else 8)


c_int_p = C.POINTER(C.c_int)
c_dbl_p = C.POINTER(C.c_double)
c_flt_p = C.POINTER(C.c_float)


class SparshError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"sparsh error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """``sparsh_params`` (include/sparsh_amg.h); defaults = macros of the reference's AMG.hpp:15-27."""

    _fields_ = [
        ("omega", C.c_double),
        ("tol", C.c_double),
        ("sweeps", C.c_int),
        ("max_levels", C.c_int),
        ("limit_upper", C.c_int),
        ("limit_lower", C.c_int),
        ("coarsening", C.c_int),
        ("max_iter", C.c_int),
        ("coarse_limit", C.c_int),
        ("host_threads", C.c_int),
        ("device", C.c_int),
        ("print_setup", C.c_int),
        ("print_solve", C.c_int),
        ("check_every", C.c_int),
        ("use_graph", C.c_int),
        ("replicate_rows", C.c_int),
        ("precond_fp32", C.c_int),
        ("dense_limit", C.c_int),
        ("extend_until", C.c_int),
        ("coarse_factor_mb", C.c_int),
    ]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C sparsh_amg_amd/csrc`).  There is no pure-Python/CPU fallback."
        )
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    P = C.POINTER
    sig = {
        "sparsh_last_error": (C.c_char_p, []),
        "sparsh_version": (C.c_int, []),
        "sparsh_device_count": (C.c_int, []),
        "sparsh_host_cpus": (C.c_int, []),
        "sparsh_default_params": (None, [P(Params)]),
        "sparsh_create_csr": (C.c_int, [C.c_int, C.c_int, c_int_p, c_int_p, c_dbl_p, P(H)]),
        "sparsh_destroy": (None, [H]),
        "sparsh_setup": (C.c_int, [H, P(Params)]),
        "sparsh_setup_host": (C.c_int, [H, P(Params)]),
        "sparsh_set_stopping": (C.c_int, [H, C.c_double, C.c_int, C.c_int]),
        "sparsh_set_kernel_config": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sparsh_level_placement": (C.c_int, [H, C.c_int, c_int_p, c_int_p]),
        "sparsh_level_format": (C.c_int, [H, C.c_int, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_level_layout": (C.c_int, [H, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "sparsh_set_const_slots": (C.c_int, [H, C.c_int]),
        "sparsh_set_tile": (C.c_int, [H, C.c_int]),
        "sparsh_set_index_compression": (C.c_int, [H, C.c_int]),
        "sparsh_set_alternate_sweeps": (C.c_int, [H, C.c_int]),
        "sparsh_set_paired_restriction": (C.c_int, [H, C.c_int]),
        "sparsh_set_fused_prolongation": (C.c_int, [H, C.c_int]),
        "sparsh_set_constant_diagonal": (C.c_int, [H, C.c_int]),
        "sparsh_set_double_sweep": (C.c_int, [H, C.c_int]),
        "sparsh_set_marching_ops": (C.c_int, [H, C.c_int]),
        "sparsh_set_zero_start": (C.c_int, [H, C.c_int]),
        "sparsh_set_deferred_x": (C.c_int, [H, C.c_int]),
        "sparsh_level_marching_ops": (C.c_int, [H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "sparsh_level_double_sweep": (C.c_int, [H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double)]),
        "sparsh_level_constant_diagonal": (C.c_int, [H, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
        "sparsh_level_prolong_fused": (C.c_int, [H, C.c_int, C.POINTER(C.c_int)]),
        "sparsh_op_jacobi_prolong": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_set_box_plan": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sparsh_set_box_plan_ex": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
        "sparsh_level_box_threads": (C.c_int, [H, C.c_int, c_int_p, c_int_p]),
        "sparsh_set_box_exact_fma": (C.c_int, [H, C.c_int]),
        "sparsh_level_box_exact_fma": (C.c_int, [H, C.c_int, c_int_p, c_int_p]),
        "sparsh_debug_box_exact_offdiag": (C.c_int, [c_dbl_p]),
        "sparsh_debug_box_plan_candidates": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int_p]),
        "sparsh_op_spmv_dot": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_jacobi_dot": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_level_paired": (C.c_int, [H, C.c_int, C.POINTER(C.c_int)]),
        "sparsh_set_fused_zero_sweep": (C.c_int, [H, C.c_int]),
        "sparsh_set_placement_search": (C.c_int, [H, C.c_int]),
        "sparsh_placement_info": (C.c_int, [H, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), c_int_p, C.POINTER(C.c_double)]),
        "sparsh_debug_index16_roundtrip": (C.c_int, [C.c_int, c_int_p, c_int_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "sparsh_set_setup_broadcast": (C.c_int, [H, C.c_int]),
        "sparsh_debug_hierarchy_roundtrip": (C.c_long, [H, C.c_long]),
        "sparsh_setup_share_info": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_long)]),
        "sparsh_level_index16": (C.c_int, [H, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "sparsh_level_tile_rows": (C.c_int, [H, C.c_int, c_int_p]),
        "sparsh_bench_comm": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_dbl_p]),
        "sparsh_level_kernel": (C.c_char_p, [H, C.c_int]),
        "sparsh_num_levels": (C.c_int, [H]),
        "sparsh_level_info": (C.c_int, [H, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p]),
        "sparsh_level_csr": (C.c_int, [H, C.c_int, C.c_int, c_int_p, c_int_p, c_dbl_p]),
        "sparsh_coarse_inverse": (C.c_int, [H, c_dbl_p]),
        "sparsh_op_precond_f32": (C.c_int, [H, c_dbl_p, c_dbl_p]),
        "sparsh_level_f32_layout": (C.c_int, [H, C.c_int, c_int_p]),
        "sparsh_op_jacobi_f32": (C.c_int, [H, C.c_int, c_flt_p, c_flt_p, C.c_int, C.c_int]),
        "sparsh_op_residual_f32": (C.c_int, [H, C.c_int, c_flt_p, c_flt_p, c_flt_p]),
        "sparsh_op_restrict_f32": (C.c_int, [H, C.c_int, c_flt_p, c_flt_p]),
        "sparsh_op_prolong_f32": (C.c_int, [H, C.c_int, c_flt_p, c_flt_p]),
        "sparsh_op_coarse_f32": (C.c_int, [H, c_flt_p, c_flt_p]),
        "sparsh_op_cvt_f32": (C.c_int, [H, C.c_long, c_dbl_p, c_flt_p]),
        "sparsh_op_cvt_f2d_dot": (C.c_int, [H, C.c_int, c_flt_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_coarse_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_coarse_window": (C.c_int, [H, c_int_p]),
        "sparsh_set_coarse_interface": (C.c_int, [H, C.c_int]),
        "sparsh_set_coarse_block": (C.c_int, [H, C.c_int]),
        "sparsh_set_coarse_form": (C.c_int, [H, C.c_int, C.c_int, C.c_int]),
        "sparsh_coarse_nd_info": (C.c_int, [H, c_int_p]),
        "sparsh_coarse_pivot_info": (C.c_int, [H, c_int_p]),
        "sparsh_set_coarse_top_merge": (C.c_int, [H, C.c_int]),
        "sparsh_setup_seconds": (C.c_double, [H]),
        "sparsh_vcycle": (C.c_int, [H, c_dbl_p, c_dbl_p, C.c_int, c_dbl_p, C.c_int, c_int_p]),
        "sparsh_vcycle_dev": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_int, c_dbl_p, C.c_int, c_int_p]),
        "sparsh_solve": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, C.c_int, c_int_p]),
        "sparsh_solve_dev": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, C.c_int, c_dbl_p, C.c_int, c_int_p, c_dbl_p]),
        "sparsh_set_device": (C.c_int, [C.c_int]),
        "sparsh_comm_unique_id": (C.c_int, [C.c_char_p]),
        "sparsh_comm_init_rccl": (C.c_int, [H, C.c_char_p, C.c_int, C.c_int]),
        "sparsh_local_range": (C.c_int, [H, C.c_int, c_int_p, c_int_p, c_int_p]),
        "sparsh_set_overlap": (C.c_int, [H, C.c_int]),
        "sparsh_comm_group_create": (C.c_int, [C.c_int, P(C.c_void_p)]),
        "sparsh_comm_group_destroy": (None, [C.c_void_p]),
        "sparsh_set_deep_halo": (C.c_int, [H, C.c_int]),
        "sparsh_dist_deep_op": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int_p]),
        "sparsh_dist_deep_op_get": (C.c_int, [H, c_int_p, c_int_p, c_dbl_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]),
        "sparsh_deep_info": (C.c_int, [H, C.c_int, c_int_p]),
        "sparsh_deep_layer_end": (C.c_int, [H, C.c_int, C.c_int, c_int_p]),
        "sparsh_deep_prefix_spmv": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_exchanges_issued": (C.c_long, [H]),
        "sparsh_comm_group_fail_after": (C.c_int, [C.c_void_p, C.c_int]),
        "sparsh_comm_group_set_delay": (C.c_int, [C.c_void_p, C.c_double]),
        "sparsh_set_comm_tuning": (C.c_int, [H, C.c_int]),
        "sparsh_comm_schedule": (C.c_int, [H, C.c_int, c_int_p, c_dbl_p]),
        "sparsh_comm_measured": (C.c_int, [H, c_dbl_p]),
        "sparsh_plan_comm_schedule": (C.c_int, [H, C.c_int, c_dbl_p]),
        "sparsh_comm_init_group": (C.c_int, [H, C.c_void_p, C.c_int]),
        "sparsh_dist_local_op": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int, c_int_p]),
        "sparsh_dist_local_op_get": (C.c_int, [H, c_int_p, c_int_p, c_dbl_p, c_int_p, c_int_p, c_int_p, c_int_p]),
        "sparsh_krylov_init_dev": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p]),
        "sparsh_krylov_step_dev": (C.c_int, [H, C.c_int, c_int_p, c_dbl_p]),
        "sparsh_krylov_history": (C.c_int, [H, c_dbl_p, C.c_int, c_int_p]),
        "sparsh_op_spmv": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_jacobi": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, C.c_int, C.c_int]),
        "sparsh_op_residual": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_resnorm": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_restrict": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_residual_restrict": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_prolong": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_coarse": (C.c_int, [H, c_dbl_p, c_dbl_p]),
        "sparsh_op_dot": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_nrm2": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_axpby": (C.c_int, [H, C.c_int, C.c_double, c_dbl_p, C.c_double, c_dbl_p]),
        "sparsh_bench_op": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_dbl_p]),
        "sparsh_dev_alloc": (C.c_int, [H, C.c_long, P(C.c_void_p)]),
        "sparsh_dev_free": (C.c_int, [H, C.c_void_p]),
        "sparsh_dev_fill": (C.c_int, [H, C.c_void_p, C.c_long, C.c_double]),
        "sparsh_h2d": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_long]),
        "sparsh_d2h": (C.c_int, [H, C.c_void_p, C.c_void_p, C.c_long]),
        "sparsh_sync": (C.c_int, [H]),
        "sparsh_profile": (C.c_int, [H, C.c_int]),
        "sparsh_set_smoother": (C.c_int, [H, C.c_int, C.c_int, C.c_int]),
        "sparsh_level_colors": (C.c_int, [H, C.c_int, c_int_p, c_int_p]),
        "sparsh_level_color_of_rows": (C.c_int, [H, C.c_int, c_int_p]),
        "sparsh_op_sor": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, C.c_int, C.c_int, C.c_int]),
        "sparsh_set_sor_path": (C.c_int, [H, C.c_int]),
        "sparsh_level_sor_layout": (C.c_int, [H, C.c_int, c_int_p, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_set_chebyshev": (C.c_int, [H, C.c_double, C.c_int]),
        "sparsh_set_chebyshev_lmax": (C.c_int, [H, C.c_int, C.c_double]),
        "sparsh_level_chebyshev": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_cheby": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, C.c_int, C.c_int]),
        "sparsh_profile_read": (C.c_int, [H, c_dbl_p]),
        "sparsh_set_cycle": (C.c_int, [H, C.c_int, C.c_int]),
        "sparsh_cycle_info": (C.c_int, [H, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "sparsh_level_cycle": (C.c_int, [H, C.c_int, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_op_kstep": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_set_nullspace": (C.c_int, [H, C.c_int]),
        "sparsh_nullspace_info": (C.c_int, [H, c_int_p, c_int_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_project": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_project_dot": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_project_dev": (C.c_int, [H, C.c_int, C.c_void_p, C.c_void_p, c_dbl_p, c_dbl_p]),
        "sparsh_set_gmres": (C.c_int, [H, C.c_int]),
        "sparsh_gmres_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_set_gmres_basis": (C.c_int, [H, C.c_int]),
        "sparsh_gmres_basis": (C.c_int, [H, c_int_p]),
        "sparsh_op_precond": (C.c_int, [H, c_dbl_p, c_dbl_p]),
        "sparsh_solve_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_long, c_dbl_p, C.c_long, c_dbl_p, C.c_int, c_int_p, c_int_p]),
        "sparsh_solve_multi_dev": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, c_dbl_p, C.c_int,
                                             c_int_p, c_int_p, c_dbl_p]),
        "sparsh_multi_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_bcg_info": (C.c_int, [H, c_int_p, c_int_p, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_debug_bcg_small": (C.c_int, [C.c_int, c_dbl_p, c_dbl_p, C.c_double, c_dbl_p, c_int_p]),
        "sparsh_op_bcg_small": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, C.c_double, c_dbl_p, c_int_p]),
        "sparsh_op_bcg_update": (C.c_int, [H, C.c_int, C.c_int] + [c_dbl_p] * 8),
        "sparsh_op_bcg_dir": (C.c_int, [H, C.c_int, C.c_int] + [c_dbl_p] * 4),
        "sparsh_mbicg_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_op_dot2_multi": (C.c_int, [H, C.c_int, C.c_int] + [c_dbl_p] * 6 + [c_int_p]),
        "sparsh_op_bicg_s_multi": (C.c_int, [H, C.c_int, C.c_int, c_int_p] + [c_dbl_p] * 4),
        "sparsh_op_bicg_xr_multi": (C.c_int, [H, C.c_int, C.c_int, c_int_p] + [c_dbl_p] * 11 + [c_int_p]),
        "sparsh_op_bicg_p_multi": (C.c_int, [H, C.c_int, C.c_int, c_int_p] + [c_dbl_p] * 5),
        "sparsh_op_mbicg_finalize": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_int, c_dbl_p, C.c_int, c_dbl_p, c_int_p, c_int_p, c_int_p,
                                               C.c_double, c_dbl_p, C.c_int, C.c_int]),
        "sparsh_op_spmv_dot_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_residual_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_jacobi_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, C.c_int, C.c_int]),
        "sparsh_op_restrict_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_prolong_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_coarse_multi": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_precond_multi": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_bench_op_multi": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.c_int, c_dbl_p]),
        "sparsh_eigs": (C.c_int, [H, C.c_int, c_dbl_p, C.c_long, C.c_double, C.c_int, c_dbl_p, c_dbl_p, C.c_int, c_int_p, c_int_p]),
        "sparsh_eigs_dev": (C.c_int, [H, C.c_int, C.c_void_p, C.c_long, C.c_double, C.c_int, c_dbl_p, c_dbl_p, C.c_int, c_int_p, c_int_p,
                                      c_dbl_p]),
        "sparsh_eig_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long), c_int_p]),
        "sparsh_debug_eig_small": (C.c_int, [C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_gram_multi": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_eig_residual": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_eig_update": (C.c_int, [H, C.c_int, C.c_int] + [c_dbl_p] * 13),
        "sparsh_eig_set_b": (C.c_int, [H, c_int_p, c_int_p, c_dbl_p]),
        "sparsh_eig_b_info": (C.c_int, [H, c_int_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "sparsh_eig_con_set_b": (C.c_int, [H, c_int_p, c_int_p, c_dbl_p]),
        "sparsh_eigs_gen": (C.c_int, [H, C.c_int, c_dbl_p, C.c_long, C.c_double, C.c_int, c_dbl_p, c_dbl_p, C.c_int, c_int_p, c_int_p]),
        "sparsh_eigs_gen_dev": (C.c_int, [H, C.c_int, C.c_void_p, C.c_long, C.c_double, C.c_int, c_dbl_p, c_dbl_p, C.c_int, c_int_p, c_int_p,
                                          c_dbl_p]),
        "sparsh_eigs_con": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_long, C.c_int, c_dbl_p, C.c_long, C.c_double, C.c_int, c_dbl_p,
                                      c_dbl_p, C.c_int, c_int_p, c_int_p]),
        "sparsh_eigs_con_dev": (C.c_int, [H, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_double, C.c_int,
                                          c_dbl_p, c_dbl_p, C.c_int, c_int_p, c_int_p, c_dbl_p]),
        "sparsh_eig_con_info": (C.c_int, [H, c_int_p, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_op_eig_con_project": (C.c_int, [H, C.c_int, C.c_int, C.c_int] + [c_dbl_p] * 6),
        "sparsh_op_eig_b_multi": (C.c_int, [H, C.c_int, c_dbl_p, c_dbl_p]),
        "sparsh_op_eig_residual_gen": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_eig_update_gen": (C.c_int, [H, C.c_int, C.c_int, C.POINTER(c_dbl_p), c_dbl_p, c_dbl_p, c_dbl_p, C.POINTER(c_dbl_p)]),
        "sparsh_set_eig_options": (C.c_int, [H, C.c_int, C.c_int]),
        "sparsh_eig_options": (C.c_int, [H, c_int_p, c_int_p]),
        "sparsh_eig_ortho_info": (C.c_int, [H, c_int_p, c_int_p, C.POINTER(C.c_long)]),
        "sparsh_debug_eig_chol": (C.c_int, [C.c_int, c_dbl_p, c_int_p, c_dbl_p, c_int_p]),
        "sparsh_op_eig_chol_small": (C.c_int, [H, C.c_int, c_dbl_p, c_int_p, c_dbl_p, c_int_p]),
        "sparsh_op_eig_transform": (C.c_int, [H, C.c_int, C.c_int, C.c_int, C.POINTER(c_dbl_p), c_dbl_p]),
        "sparsh_op_eig_ortho_apply": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_int_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_eig_active_mask": (C.c_int, [H, C.c_int, C.c_int, C.c_double, c_dbl_p, c_dbl_p, c_dbl_p, c_int_p]),
        "sparsh_op_gs_dot": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_dbl_p, c_dbl_p, C.c_int, c_dbl_p]),
        "sparsh_op_gs_update": (C.c_int, [H, C.c_int, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                          c_dbl_p, c_dbl_p, c_dbl_p, c_int_p]),
        "sparsh_op_gs_scale": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_double, c_dbl_p, c_dbl_p, c_dbl_p, c_int_p]),
        "sparsh_op_gmres_small": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p, C.c_double, C.c_int, c_dbl_p, c_dbl_p, c_dbl_p,
                                            c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_dot2": (C.c_int, [H, C.c_int] + [c_dbl_p] * 6 + [c_int_p]),
        "sparsh_op_cg_update": (C.c_int, [H, C.c_int, C.c_double, C.c_double] + [c_dbl_p] * 5 + [c_int_p, C.c_int, c_dbl_p, C.c_double,
                                          C.c_double, C.c_int, c_dbl_p]),
        "sparsh_op_p_update": (C.c_int, [H, C.c_int, C.c_double, c_dbl_p, c_dbl_p]),
        "sparsh_op_xp_update": (C.c_int, [H, C.c_int, C.c_double, C.c_double, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_bicg_s": (C.c_int, [H, C.c_int, C.c_double, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_bicg_xr": (C.c_int, [H, C.c_int, C.c_double, C.c_double] + [c_dbl_p] * 9 + [c_int_p]),
        "sparsh_op_bicg_p": (C.c_int, [H, C.c_int, C.c_double, C.c_double, c_dbl_p, c_dbl_p, c_dbl_p]),
        "sparsh_op_finalize": (C.c_int, [H, C.c_int, C.c_int, c_dbl_p, C.c_int, c_dbl_p, C.c_int, c_dbl_p, C.c_int, c_dbl_p, C.c_int,
                                         C.c_int, c_int_p, C.c_int]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    return L


lib = _load()


def _dp(a):
    return a.ctypes.data_as(c_dbl_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


def _fp(a):
    return a.ctypes.data_as(c_flt_p)


def _f32(a, copy=False):
    """A float32 vector as the float entry points take it.  Other dtypes are refused, not converted: a hidden rounding of a float64
    argument is what these entry points exist to rule out."""
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise TypeError(f"the fp32 entry points take float32 arrays, not {a.dtype}")
    return np.array(a, dtype=np.float32) if copy else np.ascontiguousarray(a)


def _check(rc, allow=()):
    if rc != SPARSH_OK and rc not in allow:
        raise SparshError(rc, lib.sparsh_last_error().decode())
    return rc


OP_PAD, OP_PARTIALS, OP_SCALARS = 4, 2048, 18  # SPARSH_OP_PAD, SPARSH_OP_PARTIALS, SPARSH_OP_SCALARS of sparsh_amg.h
OP_SENTINEL = -7.25  # what the padding of a written array holds when it goes to the device


class _OpArrays:
    """The host arrays of one sparsh_op_* call of the Krylov kernels: written arguments become padded copies, and an object given for
    several arguments maps to one array (so to one device vector)."""

    def __init__(self):
        self._seen = {}  # id -> (the object, kept alive; the array handed to the library)

    def written(self, v):
        a = np.concatenate([np.asarray(v, dtype=np.float64).ravel(), np.full(OP_PAD, OP_SENTINEL)])
        self._seen[id(v)] = (v, a)
        return a

    def partials(self):
        return self.written(np.full(OP_PARTIALS, OP_SENTINEL))

    def read(self, v):
        if id(v) not in self._seen:
            self._seen[id(v)] = (v, np.ascontiguousarray(v, dtype=np.float64))
        return self._seen[id(v)][1]


def default_params(**kw) -> Params:
    p = Params()
    lib.sparsh_default_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(f"sparsh_params has no field {k}")
        setattr(p, k, v)
    return p


def set_device(device: int):
    _check(lib.sparsh_set_device(device))


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(lib.sparsh_comm_unique_id(buf))
    return buf.raw


def comm_group_create(nranks: int):
    g = C.c_void_p()
    _check(lib.sparsh_comm_group_create(nranks, C.byref(g)))
    return g


def comm_group_destroy(g):
    lib.sparsh_comm_group_destroy(g)


def comm_group_set_delay(g, microseconds: float):
    """In-process test transport: every transport call first occupies the caller's stream this long (a slow link)."""
    _check(lib.sparsh_comm_group_set_delay(g, float(microseconds)))


def comm_group_fail_after(g, ncalls: int):
    """Fault injection (tests): every rank's halo exchange number `ncalls` and all later ones fail."""
    _check(lib.sparsh_comm_group_fail_after(g, int(ncalls)))


def index16_roundtrip(rowptr, colindex):
    """Test hook (host only): (row blocks in 16-bit delta form, row blocks) of a CSR pattern; raises if the form does not decode
    back to colindex."""
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    ci = np.ascontiguousarray(colindex, dtype=np.int32)
    a, b = C.c_long(), C.c_long()
    _check(lib.sparsh_debug_index16_roundtrip(len(rp) - 1, _ip(rp), _ip(ci), C.byref(a), C.byref(b)))
    return a.value, b.value


def box_plan_candidates(kernel, nx, ny, nz, part_cap=0):
    """Debug hook (host only): the launch plans (threads, q, ty, cz) the setup would time for the double sweep (kernel 2 or "double")
    or the plane-marching kernel (1 or "marching") on an nx x ny x nz box, the planner's plan first; part_cap > 0 bounds the marching
    kernel's workgroups."""
    k = {"double": 2, "marching": 1}.get(kernel, kernel)
    cap = 64
    buf = (C.c_int * (4 * cap))()
    n = lib.sparsh_debug_box_plan_candidates(int(k), int(nx), int(ny), int(nz), int(part_cap), cap, buf)
    if n < 0:
        raise ValueError("kernel must be 2 (double sweep) or 1 (plane-marching kernel)")
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(min(n, cap))]


def box_exact_offdiag(c):
    """Debug hook (host only): whether the six off-diagonal constants of the 7-point stencil c = (-plane, -line, -1, diagonal, +1, +line,
    +plane) are each 0 or +-2^k, k >= 0 -- the rule under which the box kernels fuse their off-diagonal terms (set_box_exact_fma)."""
    c = np.ascontiguousarray(c, dtype=np.float64)
    if c.shape != (7,):
        raise ValueError("seven stencil constants")
    return bool(lib.sparsh_debug_box_exact_offdiag(_dp(c)))


def eig_small(GA, GB, k):
    """Debug hook (host only): the Rayleigh-Ritz step of the eigensolver on the pencil (GA, GB) of order m <= 24.  Returns
    (breakdown, theta[k], C (m, k))."""
    GA, GB = np.ascontiguousarray(GA, dtype=np.float64), np.ascontiguousarray(GB, dtype=np.float64)
    m = GA.shape[0]
    if GA.shape != (m, m) or GB.shape != (m, m):
        raise ValueError("GA and GB are square matrices of one order")
    theta, Cm = np.zeros(max(int(k), 1)), np.zeros((m, max(int(k), 1)))
    rc = _check(lib.sparsh_debug_eig_small(m, int(k), _dp(GA), _dp(GB), _dp(theta), _dp(Cm)), allow=(1,))
    return rc, theta, Cm


def eig_chol(G, mask=None):
    """Debug hook (host only): the small Cholesky step of the eigensolver's ortho basis on G = V^T (B V) of order m <= 8 (upper
    triangle) over the columns of the mask (None: all).  Returns (T (m, m), mask_out (m,)): V T is B-orthonormal on the kept columns."""
    G = np.ascontiguousarray(G, dtype=np.float64)
    m = G.shape[0]
    if G.shape != (m, m):
        raise ValueError("G is a square matrix")
    mi = np.ones(m, dtype=np.int32) if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
    if mi.shape != (m,):
        raise ValueError("the mask has one entry per column")
    T, mo = np.zeros((max(m, 1), max(m, 1))), np.zeros(max(m, 1), dtype=np.int32)
    _check(lib.sparsh_debug_eig_chol(m, _dp(G), _ip(mi), _dp(T), _ip(mo)))
    return T, mo


def bcg_small(G, C, sign=1.0):
    """Debug hook (host only): block CG's small solve coef = sign * pinv(G) C by LDL^T with dropped directions, G and C of order
    k <= 8.  Returns (coef (k, k), keep (k,), rank)."""
    G, Cm = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(C, dtype=np.float64)
    k = G.shape[0]
    if G.shape != (k, k) or Cm.shape != (k, k):
        raise ValueError("G and C are square matrices of one order")
    coef, keep = np.zeros((max(k, 1), max(k, 1))), np.zeros(max(k, 1), dtype=np.int32)
    rank = lib.sparsh_debug_bcg_small(k, _dp(G), _dp(Cm), float(sign), _dp(coef), _ip(keep))
    if rank < 0:
        _check(rank)
    return coef, keep, rank


def device_count() -> int:
    return lib.sparsh_device_count()


def host_cpus() -> int:
    """CPUs this process may use (affinity mask capped by the cgroup quota)."""
    return lib.sparsh_host_cpus()


class sp_matrix_mg:
    """Host CSR container named after the reference's class (include/AMG_cpu_matrix.hpp:12-51).

    Holds rowptr/colindex/val as contiguous int32/float64 numpy arrays (aliased by the native
    handle, never copied) and owns the native solver handle.
    """

    def __init__(self, rowptr, colindex, val, ncol=None):
        self.rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        self.colindex = np.ascontiguousarray(colindex, dtype=np.int32)
        self.val = np.ascontiguousarray(val, dtype=np.float64)
        self.nrow = len(self.rowptr) - 1
        self.ncol = self.nrow if ncol is None else int(ncol)
        self.nnz = int(self.rowptr[-1])
        if len(self.colindex) < self.nnz or len(self.val) < self.nnz:
            raise ValueError("colindex/val shorter than rowptr[-1]")
        h = C.c_void_p()
        _check(lib.sparsh_create_csr(self.nrow, self.ncol, _ip(self.rowptr), _ip(self.colindex), _dp(self.val), C.byref(h)))
        self._h = h
        self.params = None

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib.sparsh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- per-handle kernel / layout choices (A/B measurements; results are bitwise identical) -----
    def set_const_slots(self, enable=True):
        """Layout option read by setup(): fold constant diagonals of a slice into one scalar."""
        _check(lib.sparsh_set_const_slots(self._h, int(bool(enable))))
        return self

    def set_setup_broadcast(self, enable=True):
        """Multi-GPU: rank 0 builds the hierarchy and broadcasts it (default) / every rank builds its own; before setup."""
        _check(lib.sparsh_set_setup_broadcast(self._h, int(bool(enable))))
        return self

    def hierarchy_roundtrip(self, truncate_to=-1):
        """Test hook: hierarchy -> byte image -> hierarchy, compared array by array; returns the image size."""
        r = lib.sparsh_debug_hierarchy_roundtrip(self._h, int(truncate_to))
        if r < 0:
            _check(int(r))
        return int(r)

    def setup_share_info(self):
        """(this rank ran the host setup itself, bytes of the broadcast hierarchy image)."""
        a, b = C.c_int(), C.c_long()
        _check(lib.sparsh_setup_share_info(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), b.value

    def set_placement_search(self, enable=True):
        """Setup-time choice of the buffers that hold the finest level's sweep vectors (default on); before setup."""
        _check(lib.sparsh_set_placement_search(self._h, int(bool(enable))))
        return self

    def placement_info(self):
        """Sweep time (us) of the chosen / worst / initial buffer triple and the number of triples timed at setup."""
        a, b, c, k, t = C.c_double(), C.c_double(), C.c_double(), C.c_int(), C.c_double()
        _check(lib.sparsh_placement_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(k), C.byref(t)))
        return {"chosen_us": round(a.value, 2), "worst_us": round(b.value, 2), "initial_us": round(c.value, 2), "triples": k.value,
                "seconds": round(t.value, 3)}

    def set_fused_zero_sweep(self, enable=2):
        """PCG: cg_update also writes the zero-guess sweep of the V-cycle: 0 off, 1 fused, 2 fused + non-temporal streams (default)."""
        _check(lib.sparsh_set_fused_zero_sweep(self._h, int(enable)))
        return self

    def set_alternate_sweeps(self, mode=1):
        """Alternate the walking direction of consecutive sweeps of a smoothing leg: 0 never, 1 large streaming levels (default), 2 always."""
        _check(lib.sparsh_set_alternate_sweeps(self._h, int(mode)))
        return self

    def set_double_sweep(self, mode=1):
        """Two Jacobi sweeps per launch on box-grid levels: 0 never, 1 where the setup times it faster (default), 2 wherever a plan exists.
        Read by setup; afterwards it can be switched between 0 and the setup's value."""
        _check(lib.sparsh_set_double_sweep(self._h, int(mode)))
        return self

    def level_double_sweep(self, level):
        on = C.c_int(0)
        dims, plan = (C.c_int * 3)(), (C.c_int * 3)()
        t1, t2 = C.c_double(0.0), C.c_double(0.0)
        _check(lib.sparsh_level_double_sweep(self._h, int(level), C.byref(on), dims, plan, C.byref(t1), C.byref(t2)))
        return {"on": bool(on.value), "grid": list(dims), "points_per_thread": plan[0], "lines_per_tile": plan[1], "planes_per_chunk": plan[2],
                "two_single_sweeps_us": round(t1.value, 2), "double_sweep_us": round(t2.value, 2)}

    def set_deferred_x(self, enable=True):
        """PCG: x += alpha p rides in the direction update at the end of the iteration (p read once for both)."""
        _check(lib.sparsh_set_deferred_x(self._h, 1 if enable else 0))
        return self

    def set_zero_start(self, enable=True):
        """Double-sweep levels: a leg that starts from a zero guess runs sweeps 1 - 3 as one launch that reads only the right-hand side."""
        _check(lib.sparsh_set_zero_start(self._h, 1 if enable else 0))
        return self

    def set_marching_ops(self, mode=1):
        """SpMV + dot, last post-sweep (+ dot / + prolongation), residual + pair restriction of box-grid levels through the plane-marching
        kernel: 0 never, 1 where the setup times it faster (default), 2 wherever a plan exists.  Read by setup."""
        _check(lib.sparsh_set_marching_ops(self._h, int(mode)))
        return self

    def level_marching_ops(self, level):
        on = C.c_int(0)
        plan = (C.c_int * 3)()
        t1, t2 = C.c_double(0.0), C.c_double(0.0)
        _check(lib.sparsh_level_marching_ops(self._h, int(level), C.byref(on), plan, C.byref(t1), C.byref(t2)))
        return {"on": bool(on.value), "points_per_thread": plan[0], "lines_per_tile": plan[1], "planes_per_chunk": plan[2],
                "table_kernel_us": round(t1.value, 2), "marching_kernel_us": round(t2.value, 2)}

    def set_box_plan(self, level, kernel, q=0, ty=0, cz=0, shared_cu=False, threads=1024):
        """Test hook: launch plan (points per thread, lines per tile, planes per chunk; threads per workgroup: 256, 512 or 1024) of
        box-grid level `level`'s double sweep (kernel 2 or "double") or plane-marching kernel (1 or "marching"); q = ty = cz = 0
        restores the planner's plan (1024 threads), with shared_cu (marching kernel) its shared-CU plan.  Does not switch the kernel on; the plan in force shows in level_double_sweep /
        level_marching_ops.  SparshError (EINVAL) for a plan the kernel cannot run."""
        k = {"double": 2, "marching": 1}.get(kernel, kernel)
        if shared_cu:
            if k != 1:
                raise ValueError("shared_cu is a plan of the marching kernel")
            k = 3
        _check(lib.sparsh_set_box_plan_ex(self._h, int(level), int(k), int(threads), int(q), int(ty), int(cz)))
        return self

    def level_box_threads(self, level):
        """Threads per workgroup of the plans in force on `level`: (double sweep, marching kernel); 0 where the kernel has no plan."""
        a, b = C.c_int(0), C.c_int(0)
        _check(lib.sparsh_level_box_threads(self._h, int(level), C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_box_exact_fma(self, mode=1):
        """Box-grid levels whose off-diagonal stencil constants are all 0 or +-2^k, k >= 0: the box kernels' off-diagonal terms as one
        FMA each (same bits): 0 never, 1 where the rule holds (default).  Before or after setup."""
        _check(lib.sparsh_set_box_exact_fma(self._h, int(mode)))
        return self

    def level_box_exact_fma(self, level):
        """Whether `level`'s box kernels run the FMA instances under the current mode."""
        on, rule = C.c_int(0), C.c_int(0)
        _check(lib.sparsh_level_box_exact_fma(self._h, int(level), C.byref(on), C.byref(rule)))
        return bool(on.value)

    def set_constant_diagonal(self, enable=True):
        """Levels with one constant diagonal: the zero-guess sweeps take it as an argument instead of streaming diag[]."""
        _check(lib.sparsh_set_constant_diagonal(self._h, 1 if enable else 0))
        return self

    def level_constant_diagonal(self, level):
        """(qualifies under the current configuration, the level's first diagonal entry)."""
        f, v = C.c_int(0), C.c_double(0.0)
        _check(lib.sparsh_level_constant_diagonal(self._h, int(level), C.byref(f), C.byref(v)))
        return bool(f.value), v.value

    def set_fused_prolongation(self, enable=True):
        """The last post-sweep of a level adds its result to the finer level's iterate itself (aggregates of one or two rows)."""
        _check(lib.sparsh_set_fused_prolongation(self._h, 1 if enable else 0))
        return self

    def level_prolong_fused(self, level):
        """Whether `level`'s last post-sweep prolongates into level - 1 itself: 0 no, 1 row pairs (2J, 2J+1), 2 member records."""
        v = C.c_int(0)
        _check(lib.sparsh_level_prolong_fused(self._h, int(level), C.byref(v)))
        return v.value

    def op_jacobi_prolong(self, level, b, x, xf):
        """xf + P_{level-1} J(x) through the fused launch (levels where level_prolong_fused() is true)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        xf = np.array(xf, dtype=np.float64)
        _check(lib.sparsh_op_jacobi_prolong(self._h, int(level), _dp(b), _dp(x), _dp(xf)))
        return xf

    def set_paired_restriction(self, enable=True):
        """Residual + restriction (+ the coarse zero-guess sweep) as one launch on levels whose aggregates are the row pairs (2J, 2J+1)."""
        _check(lib.sparsh_set_paired_restriction(self._h, 1 if enable else 0))
        return self

    def level_paired(self, level):
        """Whether `level` takes the fused residual + restriction launch: 0 no, 1 row pairs (2J, 2J+1), 2 / 3 box grid paired along y / z."""
        v = C.c_int(0)
        _check(lib.sparsh_level_paired(self._h, int(level), C.byref(v)))
        return v.value

    def set_index_compression(self, mode=1):
        """16-bit delta-coded column indices for the CSR-stream family (call before setup); see sparsh_set_index_compression."""
        _check(lib.sparsh_set_index_compression(self._h, int(mode)))
        return self

    def level_index16(self, level):
        """(row blocks of the level's operator in 16-bit index form, row blocks)."""
        a, b = C.c_long(), C.c_long()
        _check(lib.sparsh_level_index16(self._h, level, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_tile(self, enable=True):
        """LDS-tiled variant of the table kernel on whole-level launches of grid stencils (default on)."""
        _check(lib.sparsh_set_tile(self._h, int(bool(enable))))
        return self

    def level_tile_rows(self, level):
        r = C.c_int(0)
        _check(lib.sparsh_level_tile_rows(self._h, level, C.byref(r)))
        return r.value

    # -- smoother ------------------------------------------------------------------------------
    def set_smoother(self, kind="jacobi", sweeps=0, order="forward"):
        """Smoother of the V-cycle: "jacobi" (default), "sor" (multicolour SOR) or "chebyshev" (polynomial in D^-1 A); sweeps per
        leg (0: params.sweeps for Jacobi, 6 for SOR; Chebyshev: the degree, 1..16, 0 = 4); order of the SOR post-smoothing:
        "forward" or "symmetric" (SPARSH_PCG needs "symmetric")."""
        k = SMOOTHERS[kind] if isinstance(kind, str) else int(kind)
        o = SOR_ORDERS[order] if isinstance(order, str) else int(order)
        _check(lib.sparsh_set_smoother(self._h, k, int(sweeps), o))
        return self

    def set_chebyshev(self, ratio=0.0, lanczos_steps=0):
        """Chebyshev smoother: lmin = lmax / ratio (> 1; 0 = the default of 30) and the Lanczos steps of the lmax estimate (1..64;
        0 = the default of 10).  A changed step count drops the computed bounds."""
        _check(lib.sparsh_set_chebyshev(self._h, float(ratio), int(lanczos_steps)))
        return self

    def set_chebyshev_lmax(self, level, lmax=0.0):
        """Force the upper spectral bound of a level (0 restores the estimate); dropped by the next setup."""
        _check(lib.sparsh_set_chebyshev_lmax(self._h, int(level), float(lmax)))
        return self

    def level_chebyshev(self, level):
        """dict(lmax, lmin, gershgorin, lanczos) of a level; needs the host setup only."""
        out = [C.c_double() for _ in range(4)]
        _check(lib.sparsh_level_chebyshev(self._h, int(level), *[C.byref(o) for o in out]))
        return dict(zip(("lmax", "lmin", "gershgorin", "lanczos"), (o.value for o in out)))

    # -- W- and K-cycles ------------------------------------------------------------------------
    def set_cycle(self, kind="v", stride=0):
        """Cycle of the preconditioner: "v" (default), "w" or "k" (Notay's K-cycle: two flexible-CG steps) at every stride-th level
        (1..8, 0 = the default of 3).  "k" is not a fixed linear operator: solve it with "fcg" (or "amg")."""
        k = CYCLES[kind.lower()] if isinstance(kind, str) else int(kind)
        _check(lib.sparsh_set_cycle(self._h, k, int(stride)))
        return self

    def cycle_info(self):
        """dict(kind, stride, nlevels_wk, level_visits, bytes): levels that recurse twice and level visits of one cycle (0 before the
        host setup), device bytes held for the cycle's extra vectors (0 until first use)."""
        k, st, nwk = C.c_int(), C.c_int(), C.c_int()
        vis, nbytes = C.c_long(), C.c_long()
        _check(lib.sparsh_cycle_info(self._h, C.byref(k), C.byref(st), C.byref(nwk), C.byref(vis), C.byref(nbytes)))
        return dict(kind={v: n for n, v in CYCLES.items()}[k.value], stride=st.value, nlevels_wk=nwk.value, level_visits=vis.value,
                    bytes=nbytes.value)

    def level_cycle(self, level):
        """(is_wk, visits) of a level under the current cycle; needs the host setup only."""
        wk, vis = C.c_int(), C.c_long()
        _check(lib.sparsh_level_cycle(self._h, int(level), C.byref(wk), C.byref(vis)))
        return bool(wk.value), vis.value

    def op_kstep(self, level, b, c, d):
        """(r, x, scal8) of the K step's own launches on a level with c and d given (host vectors); scal8 = rho1, alpha1, gamma, beta,
        alpha2, rho2, k1, k2."""
        b, c, d = (np.ascontiguousarray(a, dtype=np.float64) for a in (b, c, d))
        r, x, s = np.zeros_like(b), np.zeros_like(b), np.zeros(8)
        _check(lib.sparsh_op_kstep(self._h, int(level), _dp(b), _dp(c), _dp(d), _dp(r), _dp(x), _dp(s)))
        return r, x, s

    # -- restarted GMRES -----------------------------------------------------------------------
    # -- constant null space ---------------------------------------------------------------------
    def set_nullspace(self, kind="constant"):
        """Null space of the matrix, read by the next setup: "none" (default) or "constant" (A 1 = 0 and 1^T A = 0: pure Neumann,
        fully periodic).  Under "constant" the solvers return the solution of mean zero of A x = b - mean(b)."""
        k = NULLSPACES[kind.lower()] if isinstance(kind, str) else int(kind)
        _check(lib.sparsh_set_nullspace(self._h, k))
        return self

    def nullspace_info(self):
        """dict(kind, pinned_row, row_defect, col_defect) of the present hierarchy ("none", -1, 0, 0 before a setup)."""
        k, row = C.c_int(), C.c_int()
        rd, cd = C.c_double(), C.c_double()
        _check(lib.sparsh_nullspace_info(self._h, C.byref(k), C.byref(row), C.byref(rd), C.byref(cd)))
        return dict(kind={v: n for n, v in NULLSPACES.items()}[k.value], pinned_row=row.value, row_defect=rd.value, col_defect=cd.value)

    def _project_shifted(self, x, r, offset, r_offset):
        """the projection launches on device copies that start `offset` / `r_offset` doubles behind a 16-byte boundary"""
        n = x.size
        xd = self.dev_alloc((n + offset) * 8)
        rd = self.dev_alloc((n + r_offset) * 8) if r is not None else None
        try:
            xs = C.c_void_p(xd.value + 8 * offset)
            self.h2d(xs, x)
            rs = None
            if r is not None:
                rs = C.c_void_p(rd.value + 8 * r_offset)
                self.h2d(rs, r)
            mean, dot = C.c_double(), C.c_double()
            _check(lib.sparsh_op_project_dev(self._h, n, xs, rs, C.byref(mean), C.byref(dot)))
            out = np.empty(n)
            self.d2h(out, xs)
        finally:
            self.dev_free(xd)
            if rd is not None:
                self.dev_free(rd)
        return out, mean.value, dot.value

    def op_project(self, x, offset=0):
        """(x - mean(x), mean) through the projection kernels (any length; the handle lends its stream only).  offset = 1: the
        device vector starts 8 bytes behind a 16-byte boundary, as a caller's _dev vector may."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if offset:
            out, mean, _ = self._project_shifted(x, None, int(offset), 0)
            return out, mean
        out, mean = x.copy(), C.c_double()
        _check(lib.sparsh_op_project(self._h, out.size, _dp(out), C.byref(mean)))
        return out, mean.value

    def op_project_dot(self, z, r, offset=0, r_offset=None):
        """(z - mean(z), mean, (z - mean(z)) . r); offset / r_offset as for op_project (r_offset defaults to offset)."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        r = np.ascontiguousarray(r, dtype=np.float64)
        r_offset = offset if r_offset is None else r_offset
        if offset or r_offset:
            return self._project_shifted(z, r, int(offset), int(r_offset))
        out, mean, dot = z.copy(), C.c_double(), C.c_double()
        _check(lib.sparsh_op_project_dot(self._h, out.size, _dp(out), _dp(r), C.byref(mean), C.byref(dot)))
        return out, mean.value, dot.value

    def set_gmres(self, restart=0, basis=None):
        """Restart length of "gmres" / "pgmres": 1..64, 0 = the default of 30.  basis: "fp64" (the default of a handle) or "fp32" =
        basis vectors stored as float with all arithmetic in fp64 (sparsh_set_gmres_basis); None leaves the precision alone.
        A changed length or precision frees the basis."""
        _check(lib.sparsh_set_gmres(self._h, int(restart)))
        if basis is not None:
            _check(lib.sparsh_set_gmres_basis(self._h, GMRES_BASES[basis] if isinstance(basis, str) else int(basis)))
        return self

    def gmres_basis(self):
        """ "fp64" or "fp32": how the Krylov basis is stored"""
        p = C.c_int()
        _check(lib.sparsh_gmres_basis(self._h, C.byref(p)))
        return {v: k for k, v in GMRES_BASES.items()}[p.value]

    def gmres_info(self):
        """dict(restart, basis_bytes): basis_bytes = device bytes now held for the Krylov basis (0 until the first GMRES solve).
        A handle whose basis is stored as float reports basis="fp32" as a third entry; the default fp64 basis adds none, so the
        dict of a handle that never chose a precision is the one it has always been (gmres_basis() names either)."""
        m, nbytes = C.c_int(), C.c_long()
        _check(lib.sparsh_gmres_info(self._h, C.byref(m), C.byref(nbytes)))
        info = dict(restart=m.value, basis_bytes=nbytes.value)
        if self.gmres_basis() != "fp64":
            info["basis"] = self.gmres_basis()
        return info

    def level_colors(self, level):
        """(ncolors, rows per colour, colour of every row) of the SOR colouring of a level; colours are numbered from 1."""
        nc = C.c_int(0)
        _check(lib.sparsh_level_colors(self._h, level, C.byref(nc), None))
        counts = np.zeros(max(nc.value, 1), dtype=np.int32)
        _check(lib.sparsh_level_colors(self._h, level, C.byref(nc), _ip(counts)))
        color = np.zeros(self.level_info(level)["nrow"], dtype=np.int32)
        _check(lib.sparsh_level_color_of_rows(self._h, level, _ip(color)))
        return nc.value, counts[: nc.value], color

    def set_sor_path(self, mode=0):
        """Debug knob of the SOR legs: 0 level policy, 1 per-colour launches everywhere, 2 one launch per leg everywhere."""
        _check(lib.sparsh_set_sor_path(self._h, int(mode)))
        return self

    def level_sor_layout(self, level):
        nc, single, nbytes = C.c_int(), C.c_int(), C.c_long()
        _check(lib.sparsh_level_sor_layout(self._h, level, C.byref(nc), C.byref(single), C.byref(nbytes)))
        return dict(ncolors=nc.value, single_launch=bool(single.value), bytes=nbytes.value)

    def set_kernel_config(self, kind=3, vec=3, nt=-1, remap=-1):
        """Select the SpMV-type kernel family of this handle; see sparsh_set_kernel_config."""
        _check(lib.sparsh_set_kernel_config(self._h, int(kind), int(vec), int(nt), int(remap)))
        return self

    def level_placement(self, level):
        nt, remap = C.c_int(0), C.c_int(0)
        _check(lib.sparsh_level_placement(self._h, level, C.byref(nt), C.byref(remap)))
        return bool(nt.value), remap.value

    # -- setup -----------------------------------------------------------------------------
    def setup(self, params: Params | None = None, host_only: bool = False):
        """AMG_solver_setup_jacobi + GPU_Allocations (host_only: hierarchy only, no GPU)."""
        self.params = params if params is not None else default_params()
        fn = lib.sparsh_setup_host if host_only else lib.sparsh_setup
        _check(fn(self._h, C.byref(self.params)))
        return self

    def set_stopping(self, tol, max_iter=0, check_every=0):
        _check(lib.sparsh_set_stopping(self._h, tol, max_iter, check_every))

    @property
    def nlevels(self):
        return lib.sparsh_num_levels(self._h)

    @property
    def setup_seconds(self):
        return lib.sparsh_setup_seconds(self._h)

    def level_info(self, level):
        a = [C.c_int() for _ in range(4)]
        _check(lib.sparsh_level_info(self._h, level, *[C.byref(v) for v in a]))
        return dict(nrow=a[0].value, nnz=a[1].value, p_ncol=a[2].value, p_nnz=a[3].value)

    def level_format(self, level):
        """(kind, stored entries) of the layout the SpMV-type kernels use on this level."""
        k, e = C.c_int(), C.c_long()
        _check(lib.sparsh_level_format(self._h, level, C.byref(k), C.byref(e)))
        return k.value, e.value

    def bench_comm(self, what, level=0, reps=50):
        """Average seconds of one communication step alone (collective); -1 when there is none."""
        sec = C.c_double()
        _check(lib.sparsh_bench_comm(self._h, {"halo": 0, "allreduce": 1, "allgather": 2}[what], level, reps, C.byref(sec)))
        return sec.value

    def level_kernel(self, level):
        """Name of the kernel the SpMV-type operations of this level launch under the current config."""
        return lib.sparsh_level_kernel(self._h, level).decode()

    def level_layout(self, level):
        """(slots, value blocks, descriptor bytes) of the sliced-diagonal layout of this level; constant
        slots own no value block."""
        sl, vb, mb = C.c_long(), C.c_long(), C.c_long()
        _check(lib.sparsh_level_layout(self._h, level, C.byref(sl), C.byref(vb), C.byref(mb)))
        return sl.value, vb.value, mb.value

    def level_csr(self, level, which="A"):
        """(rowptr, colindex, val, ncol) of A, of P or of R = P^T in its stored order (the order the restriction adds in)."""
        info = self.level_info(level)
        nrow = info["p_ncol"] if which == "R" else info["nrow"]
        nnz = info["nnz"] if which == "A" else info["p_nnz"]
        rp = np.zeros(nrow + 1, dtype=np.int32)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        v = np.zeros(max(nnz, 1), dtype=np.float64)
        _check(lib.sparsh_level_csr(self._h, level, {"A": 0, "P": 1, "R": 2}[which], _ip(rp), _ip(ci), _dp(v)))
        ncol = {"A": info["nrow"], "P": info["p_ncol"], "R": info["nrow"]}[which]
        return rp, ci[:nnz], v[:nnz], ncol

    def level_scipy(self, level, which="A"):
        import scipy.sparse as sp

        rp, ci, v, ncol = self.level_csr(level, which)
        return sp.csr_matrix((v, ci, rp), shape=(len(rp) - 1, ncol))

    def coarse_inverse(self):
        n = self.level_info(self.nlevels - 1)["nrow"]
        inv = np.zeros((n, n))
        _check(lib.sparsh_coarse_inverse(self._h, _dp(inv)))
        return inv

    def coarse_info(self):
        """Form of the coarsest-level direct solver (dense inverse, nested-dissection or block-tridiagonal factors)."""
        info = (C.c_int * 6)()
        nbytes = C.c_long(0)
        _check(lib.sparsh_coarse_info(self._h, info, C.byref(nbytes)))
        win = C.c_int(0)
        _check(lib.sparsh_coarse_window(self._h, C.byref(win)))
        nd = (C.c_int * 6)()
        _check(lib.sparsh_coarse_nd_info(self._h, nd))
        piv = (C.c_int * 4)()
        _check(lib.sparsh_coarse_pivot_info(self._h, piv))
        form = "dense" if info[1] else ("nested_dissection" if nd[0] else ("block_tridiagonal" if info[3] else "not factored yet"))
        return {"rows": info[0], "dense": bool(info[1]), "form": form, "block": info[2], "nblocks": info[3], "bandwidth": info[4],
                "extended": bool(info[5]), "bytes": nbytes.value, "window": win.value,
                "nd_nodes": nd[1], "nd_levels": nd[2], "nd_max_pivot": nd[3], "nd_launches_per_solve": nd[4], "nd_leaf": nd[5],
                "pivot_steps_lds": piv[0], "row_swaps_lds": piv[1], "pivot_steps_chip": piv[2], "row_swaps_chip": piv[3]}

    def set_coarse_form(self, form="nd", leaf=0, merge_rows=-1, top_merge_rows=-1):
        """Direct solver of a coarsest level above dense_limit rows: "nd" (nested-dissection multifrontal, default) or "bt"
        (block tridiagonal, round 2's); leaf / merge_rows / top_merge_rows tune the dissection (0 / -1 = defaults).  Call before setup."""
        _check(lib.sparsh_set_coarse_form(self._h, {"nd": 0, "bt": 1}[form], int(leaf), int(merge_rows)))
        if top_merge_rows >= 0:
            _check(lib.sparsh_set_coarse_top_merge(self._h, int(top_merge_rows)))
        return self

    def set_coarse_block(self, rows=0):
        """Block size of the block-tridiagonal coarse factorisation (0 = built-in rule); call before setup."""
        _check(lib.sparsh_set_coarse_block(self._h, int(rows)))
        return self

    def set_coarse_interface(self, enable=True):
        """Interface (window) form of the block-tridiagonal coarse solve, default on; call before setup."""
        _check(lib.sparsh_set_coarse_interface(self._h, int(enable)))
        return self

    def set_comm_tuning(self, enable=True):
        """Multi-rank setups: choose the partitioned levels and the smoothing schedule from the measured transport (default on when
        replicate_rows <= 0); call before setup."""
        _check(lib.sparsh_set_comm_tuning(self._h, int(bool(enable))))
        return self

    def comm_schedule(self):
        """Per-level decision table of the measured multi-rank schedule, or None when none was made."""
        out = []
        for l in range(self.nlevels):
            info = (C.c_int * 4)()
            cost = (C.c_double * 3)()
            rc = lib.sparsh_comm_schedule(self._h, l, info, cost)
            if rc != 0:
                return None
            out.append({"level": l, "rows": info[0], "boundary_rows": info[1], "partitioned": bool(info[2]), "deep_halo": bool(info[3]),
                        "model_us_deep_halo": round(cost[0], 2), "model_us_exchange_per_sweep": round(cost[1], 2), "model_us_replicated": round(cost[2], 2)})
        return out

    def plan_comm_schedule(self, nranks, exchange_us, exchange_us_per_MB, allreduce_us, allgather_us, allgather_us_per_MB, sweep_floor_us, sweep_us_per_MB):
        """Host-only what-if: the schedule the tuner would choose for `nranks` ranks from these measurements (no device, no transport)."""
        m = (C.c_double * 7)(exchange_us, exchange_us_per_MB, allreduce_us, allgather_us, allgather_us_per_MB, sweep_floor_us, sweep_us_per_MB)
        _check(lib.sparsh_plan_comm_schedule(self._h, int(nranks), m))
        return self.comm_schedule()

    def comm_measured(self):
        m = (C.c_double * 7)()
        if lib.sparsh_comm_measured(self._h, m) != 0:
            return None
        keys = ("exchange_us", "exchange_us_per_MB", "allreduce_us", "allgather_us", "allgather_us_per_MB", "sweep_floor_us", "sweep_us_per_MB")
        return {k: round(m[i], 3) for i, k in enumerate(keys)}

    def set_deep_halo(self, enable=True):
        """Deep-halo smoothing on partitioned levels (default on; call before setup)."""
        _check(lib.sparsh_set_deep_halo(self._h, int(bool(enable))))
        return self

    def deep_info(self, level):
        info = (C.c_int * 4)()
        _check(lib.sparsh_deep_info(self._h, level, info))
        d = {"K": info[0], "rows": info[1], "cols": info[2], "npad": info[3]}
        d["layer_end"] = []
        for q in range(d["K"] + 1 if d["K"] else 0):
            e = C.c_int()
            _check(lib.sparsh_deep_layer_end(self._h, level, q, C.byref(e)))
            d["layer_end"].append(e.value)
        return d

    def deep_prefix_spmv(self, level, rows, x_ext):
        x_ext = np.ascontiguousarray(x_ext, dtype=np.float64)
        y = np.zeros(rows)
        _check(lib.sparsh_deep_prefix_spmv(self._h, level, rows, _dp(x_ext), _dp(y)))
        return y

    def exchanges_issued(self):
        return int(lib.sparsh_exchanges_issued(self._h))

    # -- multi-GPU -------------------------------------------------------------------------
    def comm_init_rccl(self, unique_id: bytes, rank: int, nranks: int):
        """Install the RCCL transport (call before setup)."""
        assert len(unique_id) == 128
        _check(lib.sparsh_comm_init_rccl(self._h, unique_id, rank, nranks))

    def comm_init_group(self, group, rank: int):
        """Install the in-process test transport (call before setup)."""
        _check(lib.sparsh_comm_init_group(self._h, group, rank))

    def set_overlap(self, enable=True):
        """Multi-GPU: overlap halo exchange with the interior slices (same results)."""
        _check(lib.sparsh_set_overlap(self._h, 1 if enable else 0))

    def local_range(self, level=0):
        lo, hi, rep = C.c_int(), C.c_int(), C.c_int()
        _check(lib.sparsh_local_range(self._h, level, C.byref(lo), C.byref(hi), C.byref(rep)))
        return lo.value, hi.value, bool(rep.value)

    def dist_local_op(self, level, which, rank, nranks):
        """Host-only planning query: (scipy local matrix, plan dict) of operator A/P/R."""
        import scipy.sparse as sp

        w = {"A": 0, "P": 1, "R": 2}[which]
        sz = (C.c_int * 8)()
        _check(lib.sparsh_dist_local_op(self._h, level, w, rank, nranks, sz))
        nrow, nnz, nloc, nhalo, nss, nrs, nsend, row0 = list(sz)
        rp = np.zeros(nrow + 1, dtype=np.int32)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        v = np.zeros(max(nnz, 1))
        hg = np.zeros(max(nhalo, 1), dtype=np.int32)
        si = np.zeros(max(nsend, 1), dtype=np.int32)
        ss = np.zeros(max(3 * nss, 1), dtype=np.int32)
        rs = np.zeros(max(3 * nrs, 1), dtype=np.int32)
        _check(lib.sparsh_dist_local_op_get(self._h, _ip(rp), _ip(ci), _dp(v), _ip(hg), _ip(si), _ip(ss), _ip(rs)))
        M = sp.csr_matrix((v[:nnz], ci[:nnz], rp), shape=(nrow, nloc + nhalo))
        plan = dict(nloc=nloc, nhalo=nhalo, row0=row0, halo_global=hg[:nhalo], send_idx=si[:nsend],
                    send=ss[: 3 * nss].reshape(-1, 3), recv=rs[: 3 * nrs].reshape(-1, 3))
        return M, plan

    def dist_deep_op(self, level, rank, nranks, K, depth):
        """Host-only planning query of the deep-halo layout: (scipy local matrix, plan dict)."""
        import scipy.sparse as sp

        sz = (C.c_int * 8)()
        _check(lib.sparsh_dist_deep_op(self._h, level, rank, nranks, K, depth, sz))
        nrow, nnz, nloc, npad, nall, nss, nrs, nsend = list(sz)
        rp = np.zeros(nrow + 1, dtype=np.int32)
        ci = np.zeros(max(nnz, 1), dtype=np.int32)
        v = np.zeros(max(nnz, 1))
        gof = np.zeros(max(nall, 1), dtype=np.int32)
        le = np.zeros(K + 1, dtype=np.int32)
        si = np.zeros(max(nsend, 1), dtype=np.int32)
        ss = np.zeros(max(3 * nss, 1), dtype=np.int32)
        rs = np.zeros(max(3 * nrs, 1), dtype=np.int32)
        nrecv_max = max(nall - npad, 1)
        rpos = np.zeros(nrecv_max, dtype=np.int32)
        _check(lib.sparsh_dist_deep_op_get(self._h, _ip(rp), _ip(ci), _dp(v), _ip(gof), _ip(le), _ip(si), _ip(ss), _ip(rpos), _ip(rs)))
        M = sp.csr_matrix((v[:nnz], ci[:nnz], rp), shape=(nrow, nall))
        recv = rs[: 3 * nrs].reshape(-1, 3)
        nrecv = int(recv[:, 2].sum()) if len(recv) else 0
        plan = dict(nloc=nloc, npad=npad, nall=nall, global_of=gof[:nall], layer_end=le, send_idx=si[:nsend],
                    send=ss[: 3 * nss].reshape(-1, 3), recv=recv, recv_pos=rpos[:nrecv])
        return M, plan

    # -- solvers (host vectors) ------------------------------------------------------------
    def vcycle(self, b, x, iterations=-1, hist_cap=8192):
        b = np.ascontiguousarray(b, dtype=np.float64)
        hist = np.zeros(hist_cap)
        n = C.c_int()
        rc = _check(lib.sparsh_vcycle(self._h, _dp(b), _dp(x), iterations, _dp(hist), hist_cap, C.byref(n)), allow=(SPARSH_ENOCONV,))
        return hist[: min(n.value, hist_cap)].copy(), rc

    def solve(self, method, b, x, hist_cap=8192, allow=()):
        """allow: extra return codes handed back instead of raised (SPARSH_ENOCONV always is)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert x.dtype == np.float64 and x.flags.c_contiguous
        hist = np.zeros(hist_cap)
        n = C.c_int()
        m = _method(method)
        rc = _check(lib.sparsh_solve(self._h, m, _dp(b), _dp(x), _dp(hist), hist_cap, C.byref(n)), allow=(SPARSH_ENOCONV,) + tuple(allow))
        return hist[: min(n.value, hist_cap)].copy(), rc

    # -- device-resident path (bench) ------------------------------------------------------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        _check(lib.sparsh_dev_alloc(self._h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        _check(lib.sparsh_dev_free(self._h, p))

    def dev_fill(self, dptr, n, value=0.0):
        _check(lib.sparsh_dev_fill(self._h, dptr, n, value))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib.sparsh_h2d(self._h, dptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def d2h(self, arr, dptr):
        _check(lib.sparsh_d2h(self._h, arr.ctypes.data_as(C.c_void_p), dptr, arr.nbytes))

    def sync(self):
        _check(lib.sparsh_sync(self._h))

    def solve_dev(self, method, b_dev, x_dev, max_iters=0, hist_cap=8192):
        hist = np.zeros(hist_cap)
        n = C.c_int()
        sec = C.c_double()
        m = _method(method)
        rc = _check(
            lib.sparsh_solve_dev(self._h, m, b_dev, x_dev, max_iters, _dp(hist), hist_cap, C.byref(n), C.byref(sec)),
            allow=(SPARSH_ENOCONV,),
        )
        return hist[: min(n.value, hist_cap)].copy(), n.value, sec.value, rc

    def krylov_init_dev(self, method, b_dev, x_dev):
        m = _method(method)
        _check(lib.sparsh_krylov_init_dev(self._h, m, b_dev, x_dev))

    def krylov_step_dev(self, nsteps):
        done = C.c_int()
        res = C.c_double()
        _check(lib.sparsh_krylov_step_dev(self._h, nsteps, C.byref(done), C.byref(res)))
        return done.value, res.value

    def krylov_history(self, hist_cap=8192):
        hist = np.zeros(hist_cap)
        n = C.c_int()
        _check(lib.sparsh_krylov_history(self._h, _dp(hist), hist_cap, C.byref(n)))
        return hist[: min(n.value, hist_cap)].copy()

    def profile(self, enable=True):
        _check(lib.sparsh_profile(self._h, 1 if enable else 0))

    def profile_read(self):
        out = np.zeros(4)
        _check(lib.sparsh_profile_read(self._h, _dp(out)))
        return dict(launches=int(out[0]), seconds=out[1], nrow=int(out[2]), nnz=int(out[3]))

    def bench_op(self, op, level=0, reps=20):
        ops = {"spmv": 0, "jacobi": 1, "residual": 2, "restrict": 3, "prolong": 4, "coarse": 5, "dot": 6, "axpby": 7, "copy_int": 8,
               "jacobi_pingpong": 9, "jacobi_pingpong_resident": 10, "jacobi_double": 11, "sor": 12,
               "gmres_orth": 13, "gmres_orth_unfused": 14, "gmres_orth_fp32_basis": 15, "jacobi_dot_marching": 16,
               "chebyshev_pingpong_resident": 17, "project_dot": 18}
        sec = C.c_double()
        _check(lib.sparsh_bench_op(self._h, ops[op] if isinstance(op, str) else op, level, reps, C.byref(sec)))
        return sec.value

    # -- operators (host vectors; kernel parity tests) -------------------------------------
    def op_spmv(self, level, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.level_info(level)["nrow"])
        _check(lib.sparsh_op_spmv(self._h, level, _dp(x), _dp(y)))
        return y

    def op_jacobi(self, level, b, x, sweeps, x_is_zero=False):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.array(x, dtype=np.float64)
        _check(lib.sparsh_op_jacobi(self._h, level, _dp(b), _dp(x), sweeps, 1 if x_is_zero else 0))
        return x

    def op_sor(self, level, b, x, sweeps, reverse=False, x_is_zero=False):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.array(x, dtype=np.float64)
        _check(lib.sparsh_op_sor(self._h, level, _dp(b), _dp(x), int(sweeps), 1 if reverse else 0, 1 if x_is_zero else 0))
        return x

    def op_cheby(self, level, b, x, degree, x_is_zero=False):
        """One Chebyshev leg of `degree` steps on a level (host vectors), whatever the handle's smoother."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.array(x, dtype=np.float64)
        _check(lib.sparsh_op_cheby(self._h, int(level), _dp(b), _dp(x), int(degree), 1 if x_is_zero else 0))
        return x

    def op_residual(self, level, b, x):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        r = np.zeros_like(b)
        _check(lib.sparsh_op_residual(self._h, level, _dp(b), _dp(x), _dp(r)))
        return r

    def op_resnorm(self, level, b, x):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = C.c_double()
        _check(lib.sparsh_op_resnorm(self._h, level, _dp(b), _dp(x), C.byref(out)))
        return out.value

    def op_spmv_dot(self, level, x):
        """(A_l x, x . A_l x) through the launch PCG uses for A p and p.Ap on this level."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros(self.level_info(level)["nrow"])
        dot = C.c_double()
        _check(lib.sparsh_op_spmv_dot(self._h, int(level), _dp(x), _dp(y), C.byref(dot)))
        return y, dot.value

    def op_jacobi_dot(self, level, b, x):
        """(y, y . b), y = one Jacobi sweep of x, through the launch of the V-cycle's last post-sweep with its fused dot."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(b)
        dot = C.c_double()
        _check(lib.sparsh_op_jacobi_dot(self._h, int(level), _dp(b), _dp(x), _dp(y), C.byref(dot)))
        return y, dot.value

    def op_restrict(self, level, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        bc = np.zeros(self.level_info(level + 1)["nrow"])
        _check(lib.sparsh_op_restrict(self._h, level, _dp(r), _dp(bc)))
        return bc

    def op_residual_restrict(self, level, b, x):
        """(b_{l+1}, x_{l+1}) of the fused residual + restriction launch (levels where level_paired() is true)."""
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64)
        nc = self.level_info(level + 1)["nrow"]
        bc, xc = np.zeros(nc), np.zeros(nc)
        _check(lib.sparsh_op_residual_restrict(self._h, level, _dp(b), _dp(x), _dp(bc), _dp(xc)))
        return bc, xc

    def op_prolong(self, level, xc, xf):
        xc = np.ascontiguousarray(xc, dtype=np.float64)
        xf = np.array(xf, dtype=np.float64)
        _check(lib.sparsh_op_prolong(self._h, level, _dp(xc), _dp(xf)))
        return xf

    def op_coarse(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros_like(b)
        _check(lib.sparsh_op_coarse(self._h, _dp(b), _dp(x)))
        return x

    def op_precond_f32(self, r):
        """z = V32(r): one application of the opt-in fp32 preconditioner (needs precond_fp32=1)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(lib.sparsh_op_precond_f32(self._h, _dp(r), _dp(z)))
        return z

    # -- the steps of the fp32 cycle one at a time: float32 arrays in and out (needs precond_fp32=1 and two levels) ----------------
    def level_f32_layout(self, level):
        """"sdia" (float sliced-diagonal mirror), "csr" (float CSR values) or None (the coarsest level: no float operator)."""
        k = C.c_int()
        _check(lib.sparsh_level_f32_layout(self._h, int(level), C.byref(k)))
        return {0: None, 1: "sdia", 2: "csr"}[k.value]

    def op_jacobi_f32(self, level, b, x, sweeps, x_is_zero=False):
        b, x = _f32(b), _f32(x, copy=True)
        _check(lib.sparsh_op_jacobi_f32(self._h, int(level), _fp(b), _fp(x), int(sweeps), 1 if x_is_zero else 0))
        return x

    def op_residual_f32(self, level, b, x):
        b, x = _f32(b), _f32(x)
        r = np.zeros_like(b)
        _check(lib.sparsh_op_residual_f32(self._h, int(level), _fp(b), _fp(x), _fp(r)))
        return r

    def op_restrict_f32(self, level, r):
        r = _f32(r)
        bc = np.zeros(self.level_info(level)["p_ncol"], dtype=np.float32)
        _check(lib.sparsh_op_restrict_f32(self._h, int(level), _fp(r), _fp(bc)))
        return bc

    def op_prolong_f32(self, level, xc, xf):
        xc, xf = _f32(xc), _f32(xf, copy=True)
        _check(lib.sparsh_op_prolong_f32(self._h, int(level), _fp(xc), _fp(xf)))
        return xf

    def op_coarse_f32(self, b):
        b = _f32(b)
        x = np.zeros_like(b)
        _check(lib.sparsh_op_coarse_f32(self._h, _fp(b), _fp(x)))
        return x

    def op_cvt_f32(self, x64):
        """(float)x element by element, on the device."""
        x64 = np.ascontiguousarray(x64, dtype=np.float64)
        out = np.zeros(len(x64), dtype=np.float32)
        _check(lib.sparsh_op_cvt_f32(self._h, len(x64), _dp(x64), _fp(out)))
        return out

    def op_cvt_f2d_dot(self, z32, r64):
        """(z, z . r): z32 widened to float64 and its dot product with r64, through the launch that ends the fp32 cycle."""
        z32 = _f32(z32)
        r64 = np.ascontiguousarray(r64, dtype=np.float64)
        if len(r64) != len(z32):
            raise ValueError("z32 and r64 differ in length")
        z = np.zeros(len(z32))
        dot = C.c_double()
        _check(lib.sparsh_op_cvt_f2d_dot(self._h, len(z32), _fp(z32), _dp(r64), _dp(z), C.byref(dot)))
        return z, dot.value

    def op_precond(self, r):
        """z = M r as "pbicg" / "pgmres" apply it: the V-cycle of the current smoother from a zero guess, or the fp32 cycle."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        _check(lib.sparsh_op_precond(self._h, _dp(r), _dp(z)))
        return z

    # -- a block of up to 8 right-hand sides (arrays of shape (n, nrhs); handed over column-major) ------------------
    @staticmethod
    def _block(a, rows=None):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2:
            raise ValueError("a block is an array of shape (n, nrhs)")
        if rows is not None and a.shape[0] != rows:
            raise ValueError(f"the block has {a.shape[0]} rows, the level {rows}")
        return np.array(a, dtype=np.float64, order="F")  # a column-major copy of the caller's array

    def solve_multi(self, method, B, X, hist_cap=8192, allow=()):
        """Block AMG-PCG ("pcg") or block CG ("bcg": the columns share one search space, one iteration count for all; bcg_info()
        has the ranks) or block BiCGStab ("mbicg": unsymmetric systems, per column the arithmetic of "pbicg"): X (n, nrhs) holds the initial guesses on entry and the solutions on return.  Returns (histories, iters,
        status, rc): histories[c] = column c's residual after every iteration it ran; SPARSH_ENOCONV / SPARSH_ENUMERIC are handed
        back in rc and per column in status, other codes raise."""
        Bf, Xf = self._block(B), self._block(X)
        nrhs = Bf.shape[1]
        hist = np.zeros((max(nrhs, 1), hist_cap))
        iters, status = np.zeros(max(nrhs, 1), dtype=np.int32), np.zeros(max(nrhs, 1), dtype=np.int32)
        m = _method(method)
        rc = _check(lib.sparsh_solve_multi(self._h, m, nrhs, _dp(Bf), max(Bf.shape[0], 1), _dp(Xf), max(Xf.shape[0], 1), _dp(hist), hist_cap,
                                           _ip(iters), _ip(status)), allow=(SPARSH_ENOCONV, SPARSH_ENUMERIC) + tuple(allow))
        X[...] = Xf
        return [hist[c, : min(iters[c], hist_cap)].copy() for c in range(nrhs)], iters[:nrhs].copy(), status[:nrhs].copy(), rc

    def solve_multi_dev(self, method, nrhs, B_dev, ldb, X_dev, ldx, max_iters=0, hist_cap=8192):
        """The same on column-major device arrays (dev_alloc / h2d).  Returns (histories, iters, status, seconds, rc)."""
        hist = np.zeros((max(nrhs, 1), hist_cap))
        iters, status = np.zeros(max(nrhs, 1), dtype=np.int32), np.zeros(max(nrhs, 1), dtype=np.int32)
        sec = C.c_double()
        m = _method(method)
        rc = _check(lib.sparsh_solve_multi_dev(self._h, m, nrhs, B_dev, ldb, X_dev, ldx, max_iters, _dp(hist), hist_cap, _ip(iters),
                                               _ip(status), C.byref(sec)), allow=(SPARSH_ENOCONV, SPARSH_ENUMERIC))
        return [hist[c, : min(iters[c], hist_cap)].copy() for c in range(nrhs)], iters[:nrhs].copy(), status[:nrhs].copy(), sec.value, rc

    def multi_info(self):
        """Width in force and device bytes held by the block vectors (both 0 until the first block call)."""
        w, b = C.c_int(), C.c_long()
        _check(lib.sparsh_multi_info(self._h, C.byref(w), C.byref(b)))
        return dict(width=w.value, bytes=b.value)

    def bcg_info(self):
        """The last solve_multi("bcg", ...): iterations, the smallest rank of its Gram matrices, the directions dropped (all
        iterations together) and the device bytes of the solver's own small arrays (zeros before the first such solve)."""
        it, mr, dr, b = C.c_int(), C.c_int(), C.c_int(), C.c_long()
        _check(lib.sparsh_bcg_info(self._h, C.byref(it), C.byref(mr), C.byref(dr), C.byref(b)))
        return dict(iterations=it.value, min_rank=mr.value, dropped=dr.value, bytes=b.value)

    def op_bcg_small(self, W, G, Cm, sign=1.0):
        """Block CG's small-solve kernel at width W on k x k matrices (k <= W).  Returns (coef (k, k), keep (k,), rank)."""
        G, Cm = np.ascontiguousarray(G, dtype=np.float64), np.ascontiguousarray(Cm, dtype=np.float64)
        k = G.shape[0]
        coef, keep = np.zeros((max(k, 1), max(k, 1))), np.zeros(max(k, 1), dtype=np.int32)
        rank = lib.sparsh_op_bcg_small(self._h, int(W), k, _dp(G), _dp(Cm), float(sign), _dp(coef), _ip(keep))
        if rank < 0:
            _check(rank)
        return coef, keep, rank

    def op_bcg_update(self, X, R, P, Q, alpha, in_place=False):
        """Block CG's update kernel: (X + P alpha, R - Q alpha, [||R'_c||]); in_place: the outputs replace X and R on the device too."""
        Xf, Rf, Pf, Qf = (self._block(a) for a in (X, R, P, Q))
        n, k = Xf.shape
        al = np.ascontiguousarray(alpha, dtype=np.float64)
        Xo, Ro = (Xf, Rf) if in_place else (np.zeros_like(Xf, order="F"), np.zeros_like(Rf, order="F"))
        norms = np.zeros(k)
        _check(lib.sparsh_op_bcg_update(self._h, n, k, _dp(Xf), _dp(Rf), _dp(Pf), _dp(Qf), _dp(al), _dp(Xo), _dp(Ro), _dp(norms)))
        return Xo, Ro, norms

    def op_bcg_dir(self, Z, P, beta, in_place=False):
        """Block CG's direction kernel: Z + P beta; in_place: the output replaces P on the device too."""
        Zf, Pf = self._block(Z), self._block(P)
        n, k = Zf.shape
        be = np.ascontiguousarray(beta, dtype=np.float64)
        Po = Pf if in_place else np.zeros_like(Pf, order="F")
        _check(lib.sparsh_op_bcg_dir(self._h, n, k, _dp(Zf), _dp(Pf), _dp(be), _dp(Po)))
        return Po

    def mbicg_info(self):
        """The last solve_multi("mbicg", ...): its iterations (the largest count of a column) and the device bytes of the solver's
        own blocks (zeros before the first such solve)."""
        it, b = C.c_int(), C.c_long()
        _check(lib.sparsh_mbicg_info(self._h, C.byref(it), C.byref(b)))
        return dict(iterations=it.value, bytes=b.value)

    # the hooks of block BiCGStab's kernels: blocks of shape (n, nrhs), n free of the handle's matrix; `frozen` marks the columns a
    # launch must leave alone and the coefficients are one per column
    @staticmethod
    def _mb_cols(nrhs, frozen, *coefs):
        fr = np.zeros(nrhs, dtype=np.int32) if frozen is None else np.ascontiguousarray(frozen, dtype=np.int32)
        cs = [np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.float64), (nrhs,))) for c in coefs]
        if len(fr) != nrhs:
            raise ValueError("one frozen flag per column")
        return (fr, *cs)

    def op_dot2_multi(self, a, b, c, d):
        """(part0, part1), each of shape (W, nblk): every workgroup's shares of a_c . b_c and c_c . d_c, W = nrhs rounded up to 2, 4
        or 8 (the padding columns' shares are zeros).  Arrays that are the same object are one device block."""
        blocks = {}
        fa, fb, fc, fd = (blocks.setdefault(id(v), self._block(v)) for v in (a, b, c, d))
        n, k = fa.shape
        p0, p1 = np.zeros(SPARSH_MAX_RHS * SPARSH_MBICG_PARTIALS), np.zeros(SPARSH_MAX_RHS * SPARSH_MBICG_PARTIALS)
        nblk = C.c_int()
        _check(lib.sparsh_op_dot2_multi(self._h, n, k, _dp(fa), _dp(fb), _dp(fc), _dp(fd), _dp(p0), _dp(p1), C.byref(nblk)))
        W, g = multi_width(k), nblk.value
        return p0[: W * g].reshape(W, g).copy(), p1[: W * g].reshape(W, g).copy()

    def op_bicg_s_multi(self, alpha, R, AP, S, frozen=None):
        """S = R - alpha_c AP on the columns that are not frozen; the others keep the S given."""
        Rf, Af, Sf = self._block(R), self._block(AP), self._block(S)
        n, k = Sf.shape
        fr, al = self._mb_cols(k, frozen, alpha)
        _check(lib.sparsh_op_bicg_s_multi(self._h, n, k, _ip(fr), _dp(al), _dp(Rf), _dp(Af), _dp(Sf)))
        return Sf

    def op_bicg_xr_multi(self, alpha, omega, P1, S1, S, AS, R0, X, R, frozen=None):
        """(X, R, part0, part1): X = (X + alpha_c P1) + omega_c S1 and R = S - omega_c AS on the columns that are not frozen, and every
        workgroup's shares of R_c . R0_c and R_c . R_c, of shape (W, nblk)."""
        P1f, S1f, Sf, ASf, R0f, Xf, Rf = (self._block(v) for v in (P1, S1, S, AS, R0, X, R))
        n, k = Xf.shape
        fr, al, om = self._mb_cols(k, frozen, alpha, omega)
        p0, p1 = np.zeros(SPARSH_MAX_RHS * SPARSH_MBICG_PARTIALS), np.zeros(SPARSH_MAX_RHS * SPARSH_MBICG_PARTIALS)
        nblk = C.c_int()
        _check(lib.sparsh_op_bicg_xr_multi(self._h, n, k, _ip(fr), _dp(al), _dp(om), _dp(P1f), _dp(S1f), _dp(Sf), _dp(ASf), _dp(R0f), _dp(Xf),
                                           _dp(Rf), _dp(p0), _dp(p1), C.byref(nblk)))
        W, g = multi_width(k), nblk.value
        return Xf, Rf, p0[: W * g].reshape(W, g).copy(), p1[: W * g].reshape(W, g).copy()

    def op_bicg_p_multi(self, beta, omega, R, AP, P, frozen=None):
        """P = R + beta_c (P - omega_c AP) on the columns that are not frozen."""
        Rf, Af, Pf = self._block(R), self._block(AP), self._block(P)
        n, k = Pf.shape
        fr, be, om = self._mb_cols(k, frozen, beta, omega)
        _check(lib.sparsh_op_bicg_p_multi(self._h, n, k, _ip(fr), _dp(be), _dp(om), _dp(Rf), _dp(Af), _dp(Pf)))
        return Pf

    def op_mbicg_finalize(self, code, nrhs, part0, part1, state, tol, hist=None, it=0):
        """One finalise launch of block BiCGStab.  code: "init", "alpha", "omega" or "beta_res"; part0 / part1 (None: absent): arrays
        of shape (nrhs, n0) / (nrhs, n1), the partial sums of every column; state: dict(scal (SPARSH_MBICG_SCALARS, nrhs), frozen,
        iters, status (nrhs,)); hist: (nrhs, hist_cap) or None.  Returns (state, hist), both new."""
        W = multi_width(nrhs)

        def padded(p):
            p = np.asarray(p, dtype=np.float64)
            out = np.zeros((W, p.shape[1]))
            out[:nrhs] = p
            return out

        q0 = padded(part0)
        q1 = None if part1 is None else padded(part1)
        scal = np.zeros((SPARSH_MBICG_SCALARS, SPARSH_MAX_RHS))
        scal[:, :nrhs] = state["scal"]
        fr, its, st = (np.array(state[k], dtype=np.int32) for k in ("frozen", "iters", "status"))
        h = None if hist is None else np.array(hist, dtype=np.float64, order="C")
        _check(lib.sparsh_op_mbicg_finalize(self._h, MBICG_FIN[code] if isinstance(code, str) else int(code), nrhs, _dp(q0), q0.shape[1],
                                            None if q1 is None else _dp(q1), 0 if q1 is None else q1.shape[1], _dp(scal), _ip(fr), _ip(its),
                                            _ip(st), float(tol), None if h is None else _dp(h), 0 if h is None else h.shape[1], int(it)))
        return dict(scal=scal[:, :nrhs].copy(), frozen=fr, iters=its, status=st), h

    def op_spmv_dot_multi(self, level, X):
        """(A_l X, [x_c . (A_l x_c)]) through the block launch PCG uses for A p and p.Ap."""
        Xf = self._block(X, self.level_info(level)["nrow"])
        Y, dots = np.zeros_like(Xf, order="F"), np.zeros(Xf.shape[1])
        _check(lib.sparsh_op_spmv_dot_multi(self._h, int(level), Xf.shape[1], _dp(Xf), _dp(Y), _dp(dots)))
        return Y, dots

    def op_residual_multi(self, level, B, X):
        n = self.level_info(level)["nrow"]
        Bf, Xf = self._block(B, n), self._block(X, n)
        R = np.zeros_like(Bf, order="F")
        _check(lib.sparsh_op_residual_multi(self._h, int(level), Bf.shape[1], _dp(Bf), _dp(Xf), _dp(R)))
        return R

    def op_jacobi_multi(self, level, B, X, sweeps, x_is_zero=False):
        n = self.level_info(level)["nrow"]
        Bf, Xf = self._block(B, n), self._block(X, n)
        _check(lib.sparsh_op_jacobi_multi(self._h, int(level), Bf.shape[1], _dp(Bf), _dp(Xf), int(sweeps), 1 if x_is_zero else 0))
        return Xf

    def op_restrict_multi(self, level, R):
        Rf = self._block(R, self.level_info(level)["nrow"])
        BC = np.zeros((self.level_info(level + 1)["nrow"], Rf.shape[1]), order="F")
        _check(lib.sparsh_op_restrict_multi(self._h, int(level), Rf.shape[1], _dp(Rf), _dp(BC)))
        return BC

    def op_prolong_multi(self, level, XC, XF):
        XCf, XFf = self._block(XC, self.level_info(level + 1)["nrow"]), self._block(XF, self.level_info(level)["nrow"])
        _check(lib.sparsh_op_prolong_multi(self._h, int(level), XCf.shape[1], _dp(XCf), _dp(XFf)))
        return XFf

    def op_coarse_multi(self, B):
        Bf = self._block(B, self.level_info(self.nlevels - 1)["nrow"])
        X = np.zeros_like(Bf, order="F")
        _check(lib.sparsh_op_coarse_multi(self._h, Bf.shape[1], _dp(Bf), _dp(X)))
        return X

    def op_precond_multi(self, R):
        """Z = M R: one block V-cycle (Jacobi) from a zero guess, column c = the preconditioner applied to R[:, c]."""
        Rf = self._block(R, self.nrow)
        Z = np.zeros_like(Rf, order="F")
        _check(lib.sparsh_op_precond_multi(self._h, Rf.shape[1], _dp(Rf), _dp(Z)))
        return Z

    # -- lowest eigenpairs by AMG-preconditioned LOBPCG on the block path -----------------------------------------
    def eigs(self, k, X0=None, tol=1e-8, max_iters=0, seed=0, hist_cap=1024, guard=0):
        """The k <= 8 lowest eigenpairs of the SPD level-0 operator.  X0 (n, k): the start block (None: default_rng(seed)
        .standard_normal((n, k))).  Returns (lam, X, iters, hist, status): lam ascending, X (n, k) orthonormal Ritz vectors, iters[c] the
        iterations column c was active in, hist (k, evaluations) with hist[c, it] = ||A x_c - lam_c x_c|| at the start of iteration
        it, status[c] SPARSH_OK or SPARSH_ENOCONV (the cap; the code of the call is kept in last_eigs_rc).  Other codes raise.
        guard = g: the solve runs k + g <= 8 columns (X0, if given, has that many) with wanted = k for this call (set_eig), the handle's
        setting is restored afterwards, and the first k columns come back: the g guard vectors keep column k - 1 off the block's edge."""
        return self._eigs(lib.sparsh_eigs, k, X0, tol, max_iters, seed, hist_cap, guard)

    def _eigs(self, fn, k, X0, tol, max_iters, seed, hist_cap, guard=0):
        k, guard = int(k), int(guard)
        if guard:
            if guard < 0 or k < 1 or k + guard > SPARSH_MAX_RHS:
                raise ValueError(f"guard = {guard} with k = {k}: k >= 1, guard >= 0 and k + guard <= {SPARSH_MAX_RHS}")
            before = self.eig_options()
            self.set_eig(before["basis"], wanted=k)
            try:
                lam, X, iters, hist, status = self._eigs(fn, k + guard, X0, tol, max_iters, seed, hist_cap)
            finally:
                self.set_eig(before["basis"], wanted=before["wanted"])
            return lam[:k].copy(), np.asfortranarray(X[:, :k]), iters[:k].copy(), hist[:k].copy(), status[:k].copy()
        if X0 is None:
            X0 = np.random.default_rng(seed).standard_normal((self.nrow, max(k, 0)))
        Xf = self._block(X0)
        if Xf.shape[1] != k:
            raise ValueError(f"the start block has {Xf.shape[1]} columns, k = {k}")
        kk = max(k, 1)
        lam, hist = np.zeros(kk), np.full((kk, hist_cap), np.nan)
        iters, status = np.zeros(kk, dtype=np.int32), np.zeros(kk, dtype=np.int32)
        self.last_eigs_rc = _check(fn(self._h, k, _dp(Xf), max(Xf.shape[0], 1), float(tol), int(max_iters), _dp(lam), _dp(hist), hist_cap,
                                      _ip(iters), _ip(status)), allow=(SPARSH_ENOCONV,))
        nev = int(np.count_nonzero(~np.isnan(hist[0])))
        return lam[:k].copy(), Xf, iters[:k].copy(), hist[:k, :nev].copy(), status[:k].copy()

    def eigs_dev(self, k, X_dev, ldx, tol=1e-8, max_iters=0, hist_cap=1024):
        """The same on a column-major device array (dev_alloc / h2d): the start block in, the Ritz vectors out.  Returns
        (lam, iters, hist, status, seconds, rc)."""
        return self._eigs_dev(lib.sparsh_eigs_dev, k, X_dev, ldx, tol, max_iters, hist_cap)

    def _eigs_dev(self, fn, k, X_dev, ldx, tol, max_iters, hist_cap):
        kk = max(int(k), 1)
        lam, hist = np.zeros(kk), np.full((kk, hist_cap), np.nan)
        iters, status = np.zeros(kk, dtype=np.int32), np.zeros(kk, dtype=np.int32)
        sec = C.c_double()
        rc = _check(fn(self._h, int(k), X_dev, ldx, float(tol), int(max_iters), _dp(lam), _dp(hist), hist_cap, _ip(iters), _ip(status),
                       C.byref(sec)), allow=(SPARSH_ENOCONV,))
        nev = int(np.count_nonzero(~np.isnan(hist[0])))
        return lam[:k].copy(), iters[:k].copy(), hist[:k, :nev].copy(), status[:k].copy(), sec.value, rc

    # -- the orthonormalised basis and the guard vectors -----------------------------------------------------------
    def set_eig(self, basis="plain", wanted=0):
        """Options of eigs, eigs_gen, eigs_con and their _dev forms, kept by the handle through setup.  basis "plain" (the default loop)
        or "ortho" (W and P B-orthonormalised every iteration, the active mask decided on the device: for clustered spectra, where the
        plain loop ends at the cap).  wanted: 0 for all columns, else a solve ends once the lowest `wanted` columns have converged and
        the others come back as guard vectors.  No device needed."""
        names = {"plain": SPARSH_EIG_BASIS_PLAIN, "ortho": SPARSH_EIG_BASIS_ORTHO}
        _check(lib.sparsh_set_eig_options(self._h, names[basis] if isinstance(basis, str) else int(basis), int(wanted)))
        return self

    def eig_options(self):
        b, w = C.c_int(), C.c_int()
        _check(lib.sparsh_eig_options(self._h, C.byref(b), C.byref(w)))
        return dict(basis={SPARSH_EIG_BASIS_PLAIN: "plain", SPARSH_EIG_BASIS_ORTHO: "ortho"}[b.value], wanted=w.value)

    def eig_ortho_info(self):
        """Columns of W and of P dropped in the last solve under the ortho basis, and the device bytes the mode holds (0 under "plain")."""
        dw, dp_, b = C.c_int(), C.c_int(), C.c_long()
        _check(lib.sparsh_eig_ortho_info(self._h, C.byref(dw), C.byref(dp_), C.byref(b)))
        return dict(dropped_w=dw.value, dropped_p=dp_.value, bytes=b.value)

    def op_eig_chol_small(self, G, mask=None):
        """eig_chol through the one-wavefront kernel; G of order 2, 4 or 8."""
        G = np.ascontiguousarray(G, dtype=np.float64)
        W = G.shape[0]
        mi = np.ones(W, dtype=np.int32) if mask is None else np.ascontiguousarray(mask, dtype=np.int32)
        if G.shape != (W, W) or mi.shape != (W,):
            raise ValueError("G is W x W and the mask has W entries")
        T, mo = np.zeros((W, W)), np.zeros(W, dtype=np.int32)
        _check(lib.sparsh_op_eig_chol_small(self._h, W, _dp(G), _ip(mi), _dp(T), _ip(mo)))
        return T, mo

    def op_eig_transform(self, blocks, T):
        """[V T for V in blocks] through the transform kernel, all in place in one launch; one to three (n, k) blocks, T (k, k)."""
        n = np.shape(blocks[0])[0]
        blocks = [np.array(self._block(b, n), order="F") for b in blocks]
        k = blocks[0].shape[1]
        Tm = np.ascontiguousarray(T, dtype=np.float64)
        if not 1 <= len(blocks) <= 3 or Tm.shape != (k, k):
            raise ValueError("one to three blocks of k columns and a k x k matrix")
        ptrs = (c_dbl_p * 3)(*([_dp(b) for b in blocks] + [None] * (3 - len(blocks))))
        _check(lib.sparsh_op_eig_transform(self._h, n, k, len(blocks), ptrs, _dp(Tm)))
        return blocks

    def op_eig_ortho_apply(self, X, Cm, mask, W0, in_place=False):
        """W0 - X Cm on the columns of the mask, zeros elsewhere, through the masked subtraction kernel; in_place: W0 is replaced on the
        device."""
        n = np.shape(X)[0]
        Xf, Wf = self._block(X), np.array(self._block(W0, n), order="F")
        k = Xf.shape[1]
        Cf, mk = np.ascontiguousarray(Cm, dtype=np.float64), np.ascontiguousarray(mask, dtype=np.int32)
        if Cf.shape != (k, k) or mk.shape != (k,) or Wf.shape != Xf.shape:
            raise ValueError("X and W0 are n x k, Cm k x k, the mask k entries")
        out = Wf if in_place else np.zeros_like(Wf, order="F")
        _check(lib.sparsh_op_eig_ortho_apply(self._h, n, k, _dp(Xf), _dp(Cf), _ip(mk), _dp(Wf), _dp(out)))
        return out

    def op_eig_active_mask(self, theta, rn, tol, bn=None):
        """The active mask of step 2 as the device decides it from given norms (bn: the generalised form)."""
        th, r = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(rn, dtype=np.float64)
        b = None if bn is None else np.ascontiguousarray(bn, dtype=np.float64)
        mask = np.zeros(len(th), dtype=np.int32)
        _check(lib.sparsh_op_eig_active_mask(self._h, len(th), int(b is not None), float(tol), _dp(th), _dp(r), None if b is None else _dp(b),
                                             _ip(mask)))
        return mask

    def eig_info(self):
        """Width in force and device bytes held by the eigensolver's own blocks (both 0 until the first eigs call), and the
        restarts of the last solve."""
        w, b, r = C.c_int(), C.c_long(), C.c_int()
        _check(lib.sparsh_eig_info(self._h, C.byref(w), C.byref(b), C.byref(r)))
        return dict(width=w.value, bytes=b.value, restarts=r.value)

    # -- the generalised problem A x = lambda B x ---------------------------------------------------------------
    def set_eig_b(self, rowptr, col=None, val=None, con=False):
        """The SPD matrix B of the generalised problem as 0-based CSR with sorted columns (copied to the device); None drops it.  B lives
        until the next setup, close or set_eig_b.  con: for eigs_con only, which lets a handle set up with a null space through (eigs_gen
        refuses such a handle, and so does this call without con)."""
        fn = lib.sparsh_eig_con_set_b if con else lib.sparsh_eig_set_b
        if rowptr is None:
            _check(fn(self._h, None, None, None))
            return self
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        if col is None or val is None:  # (the library's refusal and its message)
            _check(fn(self._h, _ip(rp), None, None))
        ci, v = np.ascontiguousarray(col, dtype=np.int32), np.ascontiguousarray(val, dtype=np.float64)
        if len(rp) != self.nrow + 1 or len(ci) != len(v) or (len(rp) and rp[-1] > len(ci)):
            raise ValueError("B must have the handle's number of rows, and rowptr[-1] entries in col and val")
        _check(fn(self._h, _ip(rp), _ip(ci), _dp(v)))
        return self

    def eig_b_info(self):
        """Whether a B is set, its stored entries and the device bytes it holds (all 0 without one)."""
        s, nnz, b = C.c_int(), C.c_long(), C.c_long()
        _check(lib.sparsh_eig_b_info(self._h, C.byref(s), C.byref(nnz), C.byref(b)))
        return dict(is_set=bool(s.value), nnz=nnz.value, bytes=b.value)

    def eigs_gen(self, k, X0=None, tol=1e-8, max_iters=0, seed=0, hist_cap=1024, guard=0):
        """The k <= 8 lowest eigenpairs of A x = lam B x with the B of set_eig_b.  Arguments and results are those of eigs; X is
        B-orthonormal and hist[c, it] = ||A x_c - lam_c B x_c||."""
        return self._eigs(lib.sparsh_eigs_gen, k, X0, tol, max_iters, seed, hist_cap, guard)

    def eigs_gen_dev(self, k, X_dev, ldx, tol=1e-8, max_iters=0, hist_cap=1024):
        """eigs_dev for the generalised problem."""
        return self._eigs_dev(lib.sparsh_eigs_gen_dev, k, X_dev, ldx, tol, max_iters, hist_cap)

    # -- eigenpairs under constraints: null-space handles, more than 8 pairs ---------------------------------------
    def eigs_con(self, k, Y=None, gen=False, X0=None, tol=1e-8, max_iters=0, seed=0, hist_cap=1024, guard=0):
        """The k <= 8 lowest eigenpairs of A x = lam x (gen: of A x = lam B x with the B of set_eig_b) in the B-orthogonal complement of
        the columns of Y (n, ncon <= 16; None: no constraints).  On a handle set up with set_nullspace("constant") the constant vector
        is a constraint of its own accord: the pairs are the lowest nonzero ones, column 0 the Fiedler pair.  Returns what eigs
        returns."""
        Yf, ncon = self._constraints(Y)
        fn = lambda h, kk, X, ldx, *rest: lib.sparsh_eigs_con(h, int(bool(gen)), kk, X, ldx, ncon, None if Yf is None else _dp(Yf),
                                                             max(self.nrow, 1), *rest)
        return self._eigs(fn, k, X0, tol, max_iters, seed, hist_cap, guard)

    def eigs_con_dev(self, k, X_dev, ldx, ncon=0, Y_dev=None, ldy=0, gen=False, tol=1e-8, max_iters=0, hist_cap=1024):
        """eigs_dev under constraints: Y_dev a column-major device array of ncon columns.  Returns what eigs_dev returns."""
        fn = lambda h, kk, X, ld, *rest: lib.sparsh_eigs_con_dev(h, int(bool(gen)), kk, X, ld, int(ncon), Y_dev, int(ldy), *rest)
        return self._eigs_dev(fn, k, X_dev, ldx, tol, max_iters, hist_cap)

    def _constraints(self, Y):
        if Y is None:
            return None, 0
        Yf = self._block(Y, self.nrow)
        return (Yf, Yf.shape[1]) if Yf.shape[1] > 0 else (None, 0)

    def eig_con_info(self):
        """Constraints in force in the eigensolver's constraint blocks (the implicit constant vector of a null-space handle included),
        whether that vector is among them, and the device bytes the blocks hold: zeros until the first constrained call."""
        m, c, b = C.c_int(), C.c_int(), C.c_long()
        _check(lib.sparsh_eig_con_info(self._h, C.byref(m), C.byref(c), C.byref(b)))
        return dict(ncon_total=m.value, implicit_constant=c.value, bytes=b.value)

    def op_eig_con_project(self, Y, BY, Ginv, V, in_place=False):
        """(Vout, C): C = BY^T V (m, k) through the Gram launch and Vout = V - Y (Ginv C) through the projection kernel of the
        constrained eigensolver; Y, BY (n, m <= 17), V (n, k <= 8), any n > 0.  in_place: the block is projected in place on the device."""
        n = np.shape(V)[0]
        Vf, Yf, BYf = self._block(V), self._block(Y, n), self._block(BY, n)
        m, k = Yf.shape[1], Vf.shape[1]
        G = np.ascontiguousarray(Ginv, dtype=np.float64)
        if BYf.shape != Yf.shape or G.shape != (m, m):
            raise ValueError("Y and BY are n x m, Ginv m x m")
        out = Vf if in_place else np.zeros_like(Vf, order="F")
        Cm = np.zeros((m, k))
        _check(lib.sparsh_op_eig_con_project(self._h, n, k, m, _dp(Yf), _dp(BYf), _dp(G), _dp(Vf), _dp(out), _dp(Cm)))
        return out, Cm

    def op_eig_b_multi(self, X):
        """Y = B X through the block SpMV on the stored B."""
        Xf = self._block(X, self.nrow)
        Y = np.zeros_like(Xf, order="F")
        _check(lib.sparsh_op_eig_b_multi(self._h, Xf.shape[1], _dp(Xf), _dp(Y)))
        return Y

    def op_eig_residual_gen(self, AX, BX, theta):
        """(R, rnorms, bnorms): R = AX - BX * theta, the column norms of R and those of BX, through the generalised residual kernel."""
        Af, Bf = self._block(AX), self._block(BX, np.shape(AX)[0])
        th = np.ascontiguousarray(theta, dtype=np.float64)
        R, rn, bn = np.zeros_like(Af, order="F"), np.zeros(Af.shape[1]), np.zeros(Af.shape[1])
        _check(lib.sparsh_op_eig_residual_gen(self._h, Af.shape[0], Af.shape[1], _dp(Af), _dp(Bf), _dp(th), _dp(R), _dp(rn), _dp(bn)))
        return R, rn, bn

    def op_eig_update_gen(self, blocks, Cx, Cw, Cp, in_place=False):
        """(X', P', AX', AP', BX', BP') of the generalised update kernel from blocks = (X, W, P, AX, AW, AP, BX, BW, BP); in_place: every
        output replaces its block on the device."""
        n = np.shape(blocks[0])[0]
        blocks = [self._block(b, n) for b in blocks]
        if len(blocks) != 9:
            raise ValueError("nine blocks: X, W, P, AX, AW, AP, BX, BW, BP")
        k = blocks[0].shape[1]
        cs = [np.ascontiguousarray(c, dtype=np.float64) for c in (Cx, Cw, Cp)]
        if any(c.shape != (k, k) for c in cs):
            raise ValueError("the coefficient matrices are k x k")
        outs = [blocks[i] for i in (0, 2, 3, 5, 6, 8)] if in_place else [np.zeros_like(blocks[0], order="F") for _ in range(6)]
        pin, pout = (c_dbl_p * 9)(*[_dp(b) for b in blocks]), (c_dbl_p * 6)(*[_dp(o) for o in outs])
        _check(lib.sparsh_op_eig_update_gen(self._h, n, k, pin, *[_dp(c) for c in cs], pout))
        return tuple(outs)

    def op_gram_multi(self, U, V):
        """G = U^T V (nu x nv) through the Gram launch of the eigensolver; U (n, nu), V (n, nv), any n > 0."""
        Uf, Vf = self._block(U), self._block(V, np.shape(U)[0])
        G = np.zeros((Uf.shape[1], Vf.shape[1]))
        _check(lib.sparsh_op_gram_multi(self._h, Uf.shape[0], Uf.shape[1], _dp(Uf), Vf.shape[1], _dp(Vf), _dp(G)))
        return G

    def op_eig_residual(self, AX, X, theta):
        """(R, norms): R = AX - X * theta and its column norms through the eigensolver's residual kernel."""
        Af, Xf = self._block(AX), self._block(X, np.shape(AX)[0])
        th = np.ascontiguousarray(theta, dtype=np.float64)
        R, norms = np.zeros_like(Af, order="F"), np.zeros(Af.shape[1])
        _check(lib.sparsh_op_eig_residual(self._h, Af.shape[0], Af.shape[1], _dp(Af), _dp(Xf), _dp(th), _dp(R), _dp(norms)))
        return R, norms

    def op_eig_update(self, X, W, P, AX, AW, AP, Cx, Cw, Cp, in_place=False):
        """(X', P', AX', AP') of the eigensolver's update kernel; in_place: every output replaces its block on the device."""
        n = np.shape(X)[0]
        blocks = [self._block(b, n) for b in (X, W, P, AX, AW, AP)]
        k = blocks[0].shape[1]
        cs = [np.ascontiguousarray(c, dtype=np.float64) for c in (Cx, Cw, Cp)]
        if any(c.shape != (k, k) for c in cs):
            raise ValueError("the coefficient matrices are k x k")
        outs = [blocks[i] for i in (0, 2, 3, 5)] if in_place else [np.zeros_like(blocks[0], order="F") for _ in range(4)]
        _check(lib.sparsh_op_eig_update(self._h, n, k, *[_dp(b) for b in blocks], *[_dp(c) for c in cs], *[_dp(o) for o in outs]))
        return tuple(outs)

    def bench_op_multi(self, op, level=0, nrhs=8, reps=20):
        """Average seconds of one block launch on the level's resident block buffers: "spmv_dot" (0) or "jacobi_pingpong_resident" (1);
        on the eigensolver's resident blocks: "eig_gram" (2, the twelve-pair Gram launch with its finalise) or "eig_update" (3); with
        the generalised solver's blocks and a B set: "eig_update_gen" (4) or "eig_b_spmv" (5); after a constrained eigen solve of this
        width: "eig_con_project" (7), one projection with the constraints that solve left resident; under set_eig("ortho") with a B
        set: "eig_transform" (8, three blocks in place) or "eig_ortho_apply" (9, the masked subtraction)."""
        ops = {"spmv_dot": 0, "jacobi_pingpong_resident": 1, "eig_gram": 2, "eig_update": 3, "eig_update_gen": 4, "eig_b_spmv": 5,
               "eig_con_project": 7, "eig_transform": 8, "eig_ortho_apply": 9}
        sec = C.c_double()
        _check(lib.sparsh_bench_op_multi(self._h, ops[op] if isinstance(op, str) else op, int(level), int(nrhs), int(reps), C.byref(sec)))
        return sec.value

    def op_dot(self, x, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        out = C.c_double()
        _check(lib.sparsh_op_dot(self._h, len(x), _dp(x), _dp(y), C.byref(out)))
        return out.value

    def op_nrm2(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = C.c_double()
        _check(lib.sparsh_op_nrm2(self._h, len(x), _dp(x), C.byref(out)))
        return out.value

    def op_axpby(self, a, x, b, y):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.array(y, dtype=np.float64)
        _check(lib.sparsh_op_axpby(self._h, len(x), a, _dp(x), b, _dp(y)))
        return y

    # ---- test hooks of the GMRES kernels: n and nv come from the arrays, not from the handle's matrix
    def op_gs_dot(self, V, w, basis="fp64", ww=False):
        """(v_k . w for every row v_k of V[nv][n], w . w or None) through launch_gs_dot + launch_gs_finalize"""
        V = np.ascontiguousarray(V, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        nv, n = V.shape
        assert w.shape == (n,)
        sums = np.zeros(nv + 1)
        _check(lib.sparsh_op_gs_dot(self._h, n, nv, GMRES_BASES[basis], _dp(V), _dp(w), int(ww), _dp(sums)))
        return sums[:nv], (sums[nv] if ww else None)

    def op_gs_update(self, V, h, w_in, basis="fp64", in_place=False, dots=False, ww=False, sentinel=-7.25):
        """w_out = w_in (None: 0) - sum of h[k] V[k] through launch_gs_update: (w_out, V w_out or None, w_out . w_out or None, the
        elements of the device vector behind row n, which was filled with `sentinel`)"""
        V = np.ascontiguousarray(V, dtype=np.float64)
        h = np.ascontiguousarray(h, dtype=np.float64)
        nv, n = V.shape
        assert h.shape == (nv,)
        if w_in is not None:
            w_in = np.ascontiguousarray(w_in, dtype=np.float64)
            assert w_in.shape == (n,)
        w_out, sums, tail, ntail = np.zeros(n), np.zeros(nv + 1), np.zeros(3), C.c_int()
        _check(lib.sparsh_op_gs_update(self._h, n, nv, GMRES_BASES[basis], _dp(V), _dp(h), None if w_in is None else _dp(w_in), int(in_place),
                                       int(dots), int(ww), sentinel, _dp(w_out), _dp(sums), _dp(tail), C.byref(ntail)))
        return w_out, (sums[:nv] if dots else None), (sums[nv] if ww else None), tail[: ntail.value]

    def op_gs_scale(self, w, d, basis="fp64"):
        """v = w / d (0 when d is not > 0) through launch_gs_scale.  fp64: v.  fp32: (the float vector widened to double, its fp64 copy,
        the stored elements behind row n of the float vector)"""
        w = np.ascontiguousarray(w, dtype=np.float64)
        n = len(w)
        v, vd, tail, ntail = np.zeros(n), np.zeros(n), np.zeros(3), C.c_int()
        _check(lib.sparsh_op_gs_scale(self._h, n, GMRES_BASES[basis], _dp(w), float(d), _dp(v), _dp(vd), _dp(tail), C.byref(ntail)))
        return v if basis == "fp64" else (v, vd, tail[: ntail.value])

    def op_gmres_small(self, hcols, ccols, ww_partial, beta, k=None):
        """launch_gmres_step for j = 0..m-1 on a zeroed state, then launch_gmres_solve(k).  hcols[j], ccols[j]: the j + 1 coefficients
        of the two Gram-Schmidt passes of step j; ww_partial[m][nblk].  Returns dict(hist[m], R[m][m] upper triangular, cs, sn, g[m+1], ny[k])"""
        m = len(hcols)
        ww_partial = np.ascontiguousarray(ww_partial, dtype=np.float64)
        assert len(ccols) == m and ww_partial.ndim == 2 and ww_partial.shape[0] == m
        assert all(len(hcols[j]) == j + 1 and len(ccols[j]) == j + 1 for j in range(m))
        k = m if k is None else int(k)
        hp = np.concatenate([np.asarray(c, dtype=np.float64) for c in hcols]) if m else np.zeros(1)
        cp = np.concatenate([np.asarray(c, dtype=np.float64) for c in ccols]) if m else np.zeros(1)
        M = 64
        hist, R, cs, sn, g, ny = np.zeros(max(m, 1)), np.zeros((M, M)), np.zeros(M), np.zeros(M), np.zeros(M + 1), np.zeros(M)
        _check(lib.sparsh_op_gmres_small(self._h, m, ww_partial.shape[1], _dp(hp), _dp(cp), _dp(ww_partial), float(beta), k, _dp(hist), _dp(R),
                                         _dp(cs), _dp(sn), _dp(g), _dp(ny)))
        return dict(hist=hist[:m], R=R[:m, :m].T.copy(), cs=cs[:m], sn=sn[:m], g=g[: m + 1], ny=ny[:k])

    # ---- test hooks of the single-vector Krylov kernels and of finalize_kernel: one launch each, n comes from the arrays.  Every
    # result is a dict; "tails" holds, per written array, what the device vector held behind its logical end (it went up filled with
    # OP_SENTINEL).  An array object given for two arguments is one device vector.
    def op_dot2(self, a, b, c, d):
        """partial sums of a.b and c.d through launch_dot2: dict(p0, p1, nblk, tails)"""
        m = _OpArrays()
        p0, p1 = m.partials(), m.partials()
        a, b, c, d = (m.read(v) for v in (a, b, c, d))
        nblk = C.c_int()
        _check(lib.sparsh_op_dot2(self._h, len(a), _dp(a), _dp(b), _dp(c), _dp(d), _dp(p0), _dp(p1), C.byref(nblk)))
        k = nblk.value
        return dict(p0=p0[:k].copy(), p1=p1[:k].copy(), nblk=k, tails=dict(p0=p0[k:], p1=p1[k:]))

    def op_cg_update(self, alpha, p, Ap, x, r, nalpha=None, zero=False, d=None, dconst=1.0, omega=1.0, nt=False):
        """x += alpha p (x None: deferred), r += nalpha Ap (nalpha None: -alpha), partial sums of r.r through launch_cg_update, or with
        zero=True through launch_cg_update_zero (z0 = omega r / d, d None: dconst; nt: the nontemporal instantiation):
        dict(x, r, z0, partial, nblk, tails)"""
        m = _OpArrays()
        n = len(r)
        xo = None if x is None else m.written(x)
        ro, part = m.written(r), m.partials()
        z0 = m.written(np.zeros(n)) if zero else None
        p, Ap = m.read(p), m.read(Ap)
        d = None if d is None else m.read(d)
        nblk = C.c_int()
        ptr = lambda v: None if v is None else _dp(v)
        _check(lib.sparsh_op_cg_update(self._h, n, float(alpha), float(-alpha if nalpha is None else nalpha), _dp(p), _dp(Ap), ptr(xo), _dp(ro),
                                       _dp(part), C.byref(nblk), int(zero), ptr(d), float(dconst), float(omega), int(nt), ptr(z0)))
        k = nblk.value
        tails = dict(r=ro[n:], partial=part[k:])
        if xo is not None:
            tails["x"] = xo[n:]
        if zero:
            tails["z0"] = z0[n:]
        return dict(x=None if xo is None else xo[:n].copy(), r=ro[:n].copy(), z0=z0[:n].copy() if zero else None, partial=part[:k].copy(),
                    nblk=k, tails=tails)

    def op_p_update(self, beta, z, p):
        """p = 1.0 z + beta p through launch_p_update: dict(p, tails)"""
        m = _OpArrays()
        n = len(p)
        po = m.written(p)
        z = m.read(z)
        _check(lib.sparsh_op_p_update(self._h, n, float(beta), _dp(z), _dp(po)))
        return dict(p=po[:n].copy(), tails=dict(p=po[n:]))

    def op_xp_update(self, alpha, beta, z, p, x):
        """x += alpha p ; p = 1.0 z + beta p through launch_xp_update: dict(x, p, tails)"""
        m = _OpArrays()
        n = len(p)
        po, xo = m.written(p), m.written(x)
        z = m.read(z)
        _check(lib.sparsh_op_xp_update(self._h, n, float(alpha), float(beta), _dp(z), _dp(po), _dp(xo)))
        return dict(x=xo[:n].copy(), p=po[:n].copy(), tails=dict(x=xo[n:], p=po[n:]))

    def op_bicg_s(self, alpha, r, Ap):
        """s = r - alpha Ap through launch_bicg_s: dict(s, tails)"""
        m = _OpArrays()
        n = len(r)
        s = m.written(np.zeros(n))
        r, Ap = m.read(r), m.read(Ap)
        _check(lib.sparsh_op_bicg_s(self._h, n, float(alpha), _dp(r), _dp(Ap), _dp(s)))
        return dict(s=s[:n].copy(), tails=dict(s=s[n:]))

    def op_bicg_xr(self, alpha, omega1, p1, s1, s, As, r0, x, r):
        """x = x + alpha p1 + omega1 s1 ; r = s - omega1 As ; partial sums of r.r0 and r.r through launch_bicg_xr:
        dict(x, r, q0, q1, nblk, tails)"""
        m = _OpArrays()
        n = len(x)
        xo, ro, q0, q1 = m.written(x), m.written(r), m.partials(), m.partials()
        p1, s1, s, As, r0 = (m.read(v) for v in (p1, s1, s, As, r0))
        nblk = C.c_int()
        _check(lib.sparsh_op_bicg_xr(self._h, n, float(alpha), float(omega1), _dp(p1), _dp(s1), _dp(s), _dp(As), _dp(r0), _dp(xo), _dp(ro),
                                     _dp(q0), _dp(q1), C.byref(nblk)))
        k = nblk.value
        return dict(x=xo[:n].copy(), r=ro[:n].copy(), q0=q0[:k].copy(), q1=q1[:k].copy(), nblk=k,
                    tails=dict(x=xo[n:], r=ro[n:], q0=q0[k:], q1=q1[k:]))

    def op_bicg_p(self, beta, omega1, r, Ap, p):
        """p = r + beta (p - omega1 Ap) through launch_bicg_p: dict(p, tails)"""
        m = _OpArrays()
        n = len(p)
        po = m.written(p)
        r, Ap = m.read(r), m.read(Ap)
        _check(lib.sparsh_op_bicg_p(self._h, n, float(beta), float(omega1), _dp(r), _dp(Ap), _dp(po)))
        return dict(p=po[:n].copy(), tails=dict(p=po[n:]))

    def op_finalize(self, code, p0, p1=None, scal=None, slot=0, mode=0, hist=None, it=0, counter=0, repeat=1):
        """`repeat` launch_finalize calls of one code and mode on the partial sums p0 (None in mode 2) and p1 (or None), the scalar
        block scal (None: zeros) and the history hist (or None; its length is hist_cap); it < 0: the slot comes from the device
        counter, which starts at `counter`.  dict(scal, hist, counter, tails)"""
        sc = np.zeros(OP_SCALARS) if scal is None else np.array(scal, dtype=np.float64)
        assert sc.shape == (OP_SCALARS,)
        m = _OpArrays()
        cap = 0 if hist is None else len(hist)
        ho = None if hist is None else m.written(hist)
        p0 = None if p0 is None else m.read(p0)
        p1 = None if p1 is None else m.read(p1)
        ctr = C.c_int(int(counter))
        ptr = lambda v: None if v is None else _dp(v)
        _check(lib.sparsh_op_finalize(self._h, int(code), int(mode), ptr(p0), 1 if p0 is None else len(p0), ptr(p1), 0 if p1 is None else len(p1),
                                      _dp(sc), int(slot), ptr(ho), cap, int(it), C.byref(ctr), int(repeat)))
        return dict(scal=sc, hist=None if ho is None else ho[:cap].copy(), counter=ctr.value, tails={} if ho is None else dict(hist=ho[cap:]))



# ---- entry points named as in the reference's include/AMG.hpp:40-85 --------------------------
# Each call redoes the setup, as the reference does (solver objects live inside one call).

def _entry(method):
    def run(A: sp_matrix_mg, b, x, params: Params | None = None):
        A.setup(params)
        hist, _ = A.solve(method, b, x)
        return hist

    return run


AMG_Solver_CPU_baseline = _entry("amg")
AMG_Solver_1 = AMG_Solver_CPU_baseline
AMG_Solver_CPU_GPU_CI = _entry("amg")
AMG_Solver_CPU_GPU_MI = _entry("amg")
Solver_CG_1 = Solver_CG_2 = _entry("cg")
Solver_PCG_1 = Solver_PCG_2 = Solver_PCG_3 = Solver_PCG_4 = _entry("pcg")
Solver_BiCG_1 = _entry("bicg")
Solver_PBiCG_1 = Solver_PBiCG_2 = Solver_PBiCG_3 = Solver_PBiCG_4 = _entry("pbicg")
Solver_GMRES_1 = _entry("gmres")
Solver_PGMRES_1 = _entry("pgmres")
Solver_FCG_1 = _entry("fcg")


def readcoo(matrixfile: str, rhsfile: str):
    """Native text format of the reference (src/AMG_file_read.cpp:39-72) -> (sp_matrix_mg, b)."""
    with open(matrixfile) as f:
        nrow, ncol, nnz = (int(t) for t in f.readline().split())
        data = np.loadtxt(f, dtype=np.float64, ndmin=2)
    if data.shape[0] != nnz:
        raise IOError(f"{matrixfile}: header says {nnz} entries, file holds {data.shape[0]}")
    rows = data[:, 0].astype(np.int64)
    if np.any(np.diff(rows) < 0):
        raise IOError("readcoo requires entries sorted by row (as the reference does)")
    rowptr = np.zeros(nrow + 1, dtype=np.int32)
    np.cumsum(np.bincount(rows, minlength=nrow), out=rowptr[1:])
    with open(rhsfile) as f:
        n = int(f.readline().split()[0])
        b = np.loadtxt(f, dtype=np.float64)
    assert n == nrow
    return sp_matrix_mg(rowptr, data[:, 1].astype(np.int32), data[:, 2].copy(), ncol=ncol), b[:nrow].copy()
