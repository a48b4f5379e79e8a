"""ctypes binding of include/rapidnet.h (librapidnet_hip.so) and a thin Python controller on top of it.

There is no CPU fallback: if the HIP library is missing or fails to load this module raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

RN_F32, RN_F64 = 0, 1
(BUF_X, BUF_U, BUF_V, BUF_XI, BUF_PSI, BUF_ACC_XI, BUF_ACC_PSI, BUF_UPD_XI, BUF_UPD_PSI, BUF_PRIMAL_XI,
 BUF_PRIMAL_PSI, BUF_DUAL_XI, BUF_DUAL_PSI, BUF_RES_XI, BUF_RES_PSI, BUF_UHAT, BUF_E, BUF_BETA, BUF_ALPHA,
 BUF_XMIN, BUF_XMAX, BUF_XS, BUF_UMIN, BUF_UMAX,
 BUF_PREV_XI, BUF_PREV_PSI, BUF_LBFGS_CUR_YVEC_XI, BUF_LBFGS_CUR_YVEC_PSI, BUF_LBFGS_PREV_YVEC_XI,
 BUF_LBFGS_PREV_YVEC_PSI, BUF_LBFGS_DIR_XI, BUF_LBFGS_DIR_PSI, BUF_PRIMAL_XI_DIR, BUF_PRIMAL_PSI_DIR,
 BUF_XDIR, BUF_UDIR, BUF_CERT_X, BUF_CERT_U) = range(38)
ALG_APG, ALG_GLOBAL_FBE, ALG_NAMA = 0, 1, 2
ALGORITHMS = {"proximalAlgorithm": ALG_APG, "globalFbeAlgorithm": ALG_GLOBAL_FBE, "namaAlgorithm": ALG_NAMA}  # Engine.cu:151-163
OP_PHI, OP_PSI, OP_D, OP_F, OP_OMEGA, OP_THETA, OP_G = range(7)
OPS_DENSE, OPS_STRUCTURED, OPS_AUTO = 0, 1, 2
OPS_MODES = {"dense": OPS_DENSE, "structured": OPS_STRUCTURED, "auto": OPS_AUTO}
STORE_NATIVE, STORE_F32 = 0, 1
STORAGES = {"native": STORE_NATIVE, "f32": STORE_F32}
PAIR_OFF, PAIR_ON, PAIR_AUTO = 0, 1, 2
PAIRINGS = {"off": PAIR_OFF, "on": PAIR_ON, "auto": PAIR_AUTO}
RESTART_OFF, RESTART_GRADIENT = 0, 1   # rn_set_restart
RESTARTS = {"off": RESTART_OFF, "gradient": RESTART_GRADIENT}
STEP_FIXED, STEP_LIPSCHITZ = 0, 1       # rn_set_step_rule
STEP_RULES = {"fixed": STEP_FIXED, "lipschitz": STEP_LIPSCHITZ}
LIP_COLUMNS = ("norm", "rayleigh", "residual", "iterations")      # rn_estimate_lipschitz, RN_LIP_*
# rn_solve_certificate: the named columns of the record, in the order of RN_CERT_* (the record is padded to CERT_COLS doubles)
CERT_COLUMNS = ("dual", "primal", "gap", "cost", "inner", "support", "distX", "distS", "uExcess", "normX", "normS", "xisPos", "absTerms", "valid")
CERT_COLS = 16
BOUNDS_SHARED, BOUNDS_PER_STAGE, BOUNDS_PER_NODE = 0, 1, 2      # rn_set_bounds
BOUNDS = {"shared": BOUNDS_SHARED, "stage": BOUNDS_PER_STAGE, "node": BOUNDS_PER_NODE}
# include/rapidnet_debug.h, RN_KNOB_*
KNOBS = {k: i for i, k in enumerate(("dual_trips", "dual_pipe", "vlv_wide", "slab_pipe", "slab_frag", "unscaled_walk", "stream_two_per_cu",
                                     "stream_split", "nama_pair", "ls_sequential", "value_mfma", "tune_bias_us", "struct_linear", "fuse_split", "stream_skip", "stream_half"))}
EXCHANGE_COLLECTIVE, EXCHANGE_ONESHOT, EXCHANGE_AUTO = 0, 1, 2
# rn_plan_report: the columns of both tables, in the order of RN_PLAN_* (the first six are sums, the last three maxima)
PLAN_COLUMNS = ("econ", "smooth", "stored", "shortExp", "xboxExp", "uboxExp", "shortMax", "xboxMax", "uboxMax")
PLAN_SUMS = 6
# rn_plan_quantiles / rn_plan_paths: which array (RN_BAND_*), and the most levels one call takes
BAND_X, BAND_U, BAND_MAX_LEVELS = 0, 1, 16
BANDS = {"x": BAND_X, "u": BAND_U}

# every symbol include/rapidnet.h (the boundary) and include/rapidnet_debug.h (test hooks, rn_debug_*) declare
SYMBOLS = [
    "rn_create", "rn_destroy", "rn_last_error", "rn_synchronize", "rn_factor_step", "rn_set_tree_errors",
    "rn_set_uncertainty", "rn_update_state_control", "rn_eliminate_input_disturbance_coupling", "rn_set_parameters",
    "rn_apg_reset", "rn_apg_iterate", "rn_algorithm_apg", "rn_apg_solve", "rn_set_stop_tolerance", "rn_get_stop_tolerance", "rn_get_last_solve", "rn_set_restart", "rn_get_restart", "rn_get_restart_info", "rn_control_action", "rn_dual_extrapolation_step",
    "rn_solve_step", "rn_proximal_fun_g", "rn_compute_fixed_point_residual", "rn_dual_update",
    "rn_update_primal_infeasibility", "rn_get_prox_distances", "rn_buffer_size", "rn_get", "rn_set", "rn_get_operator",
    "rn_device_pointer", "rn_profile_enable", "rn_profile_reset", "rn_profile_read", "rn_algorithmic_bytes", "rn_stream",
    "rn_comm_unique_id", "rn_comm_init", "rn_comm_init_timeout", "rn_comm_check", "rn_comm_library", "rn_set_cut_stage", "rn_get_history_parts", "rn_get_counters", "rn_debug_sweep_phase",
    "rn_debug_cut_buffer", "rn_set_cut_children_moments", "rn_set_operator_mode", "rn_get_operator_mode", "rn_set_operator_storage", "rn_get_operator_storage", "rn_set_sweep_pairing", "rn_get_sweep_pairing", "rn_set_operator", "rn_set_operators", "rn_get_operators", "rn_set_operators_device", "rn_get_operators_device", "rn_set_warm_start", "rn_set_exchange_mode",
    "rn_measure_hbm", "rn_set_algorithm", "rn_fbe_reset", "rn_algorithm_fbe_nama", "rn_compute_hessian_oracle", "rn_compute_gradient_fbe",
    "rn_update_fixed_point_residual_nama", "rn_compute_lbfgs_direction", "rn_update_lbfgs_buffer", "rn_two_loop_recursion_lbfgs", "rn_compute_value_fbe",
    "rn_line_search_lbfgs_update", "rn_line_search_ame_lbfgs_update", "rn_lbfgs_state", "rn_lbfgs_column",
    "rn_get_range", "rn_set_range", "rn_get_kernel_info", "rn_default_cut_stage", "rn_partition_create", "rn_partition_destroy", "rn_create_sharded", "rn_shard_info", "rn_shard_global_nodes",
    "rn_debug_set_allreduce", "rn_debug_local_group_create", "rn_debug_local_group_join", "rn_debug_local_group_destroy",
    "rn_guard_check", "rn_device_memory_info", "rn_reserve_iterations", "rn_profile_read_collective", "rn_debug_inject_allocation", "rn_guard_report", "rn_debug_guard_poke",
    "rn_set_tree_data", "rn_set_tree_data_device", "rn_get_tree_data", "rn_set_bounds", "rn_set_bounds_device", "rn_get_bounds_layout", "rn_get_bounds", "rn_debug_cut_moments",
    "rn_fbe_counters", "rn_peer_inbox_create", "rn_peer_inbox_connect", "rn_debug_peer_inbox_connect_local", "rn_debug_peer_seq", "rn_set_exchange_transport", "rn_exchange_autotune", "rn_set_fused_walk_dual", "rn_debug_set_knob", "rn_debug_stream_info", "rn_debug_restart_test", "rn_debug_stream_live", "rn_debug_stream_units", "rn_debug_stream_product", "rn_debug_slab_product", "rn_debug_dual_update",
    "rn_plan_report", "rn_plan_report_scenarios", "rn_plan_report_device",
    "rn_plan_quantiles", "rn_plan_quantiles_device", "rn_plan_paths",
    "rn_shift_warm_start", "rn_set_shift_map", "rn_get_shift_map",
    "rn_estimate_lipschitz", "rn_get_lipschitz", "rn_set_step_rule", "rn_get_step_rule",
    "rn_solve_certificate", "rn_solve_certificate_device", "rn_debug_certificate_hz",
]


class RnDims(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("nx", "nu", "nv", "nd", "N", "K", "nodes", "nNonLeafNodes")]


class RnTree(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("stages", "nodesPerStage", "nodesPerStageCumul", "ancestor", "nChildren",
                                         "nChildrenCumul", "probNode")]


class RnSystem(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("matB", "matGd", "matL", "matLhat", "costW", "matDiagPrecnd", "vecXmin",
                                         "vecXmax", "vecXsafe", "vecUmin", "vecUmax", "costAlpha1")]


class RnPartition(C.Structure):
    _fields_ = [("dims", RnDims), ("tree", RnTree), ("globalNode", C.POINTER(C.c_int)), ("errorDemandNode", C.POINTER(C.c_double)),
                ("errorPriceNode", C.POINTER(C.c_double)), ("rank", C.c_int), ("nranks", C.c_int), ("cutStage", C.c_int),
                ("nCutParents", C.c_int), ("momE", C.POINTER(C.c_double)), ("momP", C.POINTER(C.c_double)), ("owner", C.c_void_p)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p)

_LIB = None


def lib_path():
    return os.environ.get("RAPIDNET_LIB") or _build.LIB_HIP


def load():
    """Load librapidnet_hip.so (must have been built: `python -m rapidnet_amd.build`)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if os.environ.get("RAPIDNET_LIB"):
        if not os.path.exists(path):
            raise RuntimeError("$RAPIDNET_LIB names a missing library: %s" % path)
    else:
        # (re)build in-tree when the library is missing or older than its sources (a no-op otherwise; hipcc is part of the
        # image).  Under a launcher only local rank 0 compiles, before any GPU call; the others wait for the finished file
        # (build_hip renames it into place).  There is no CPU fallback.
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        # left by local rank 0 when its build fails, so that the waiting ranks abort at once.  Its first line is the fingerprint of
        # the sources that failed to build: a marker an EARLIER run left behind for other sources is ignored (the waiting ranks may
        # look before local rank 0 has removed it)
        failed = path + ".buildfailed"
        try:
            if local_rank == 0:
                if os.path.exists(failed):
                    os.remove(failed)
                try:
                    _build.build_hip()
                except Exception as e:
                    with open(failed, "w") as f:
                        f.write("%s\n%s" % (_build.hip_fingerprint(), e))
                    raise
            else:
                import time

                for _ in range(1800):
                    if not _build.hip_is_stale():
                        break
                    if os.path.exists(failed):
                        try:
                            stamp, _, why = open(failed).read().partition("\n")
                        except OSError:      # removed between the two calls
                            stamp, why = "", ""
                        if stamp.strip() == _build.hip_fingerprint():
                            raise RuntimeError("local rank 0 could not build librapidnet_hip.so: %s" % why.strip())
                    time.sleep(0.5)
                else:   # every rank must run the same binary: a library that is still stale after 15 minutes is an error, not a fallback
                    raise RuntimeError("librapidnet_hip.so is still older than its sources after waiting 900 s for local rank 0 to rebuild it")
        except Exception as e:
            if local_rank != 0 or not os.path.exists(path) or int(os.environ.get("WORLD_SIZE", "1")) > 1:   # ranks never run different binaries
                raise RuntimeError("librapidnet_hip.so (%s) is missing or stale and could not be built (%s); run __graft_entry__.build() -- "
                                   "there is no CPU fallback" % (path, e))
            import warnings

            warnings.warn("librapidnet_hip.so could not be rebuilt (%s); loading the existing (possibly stale) binary" % e)
    lib = C.CDLL(path)
    vp, dp, ip = C.c_void_p, C.c_void_p, C.c_int
    lib.rn_create.argtypes = [C.POINTER(RnDims), C.POINTER(RnTree), ip, ip, C.POINTER(vp)]
    lib.rn_destroy.argtypes = [vp]
    lib.rn_last_error.argtypes = [vp]
    lib.rn_last_error.restype = C.c_char_p
    lib.rn_synchronize.argtypes = [vp]
    lib.rn_factor_step.argtypes = [vp, C.POINTER(RnSystem)]
    lib.rn_set_tree_errors.argtypes = [vp, dp, dp]
    lib.rn_set_uncertainty.argtypes = [vp, ip, ip, C.c_double]
    lib.rn_update_state_control.argtypes = [vp, dp, dp, dp]
    lib.rn_eliminate_input_disturbance_coupling.argtypes = [vp, dp, dp]
    lib.rn_set_parameters.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    lib.rn_apg_reset.argtypes = [vp]
    lib.rn_apg_iterate.argtypes = [vp, ip, dp]
    lib.rn_algorithm_apg.argtypes = [vp, ip, dp]
    lib.rn_apg_solve.argtypes = [vp, ip, C.c_double, ip, C.POINTER(C.c_int), dp]
    lib.rn_set_stop_tolerance.argtypes = [vp, C.c_double, ip]
    lib.rn_get_stop_tolerance.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.rn_get_last_solve.argtypes = [vp, dp]
    lib.rn_set_restart.argtypes = [vp, ip]
    lib.rn_get_restart.argtypes = [vp, C.POINTER(C.c_int)]
    lib.rn_get_restart_info.argtypes = [vp, dp, dp]
    lib.rn_debug_restart_test.argtypes = [vp, dp]
    lib.rn_control_action.argtypes = [vp, dp, dp, dp, dp, dp, ip, ip, dp]
    lib.rn_dual_extrapolation_step.argtypes = [vp, C.c_double]
    for f in ("rn_solve_step", "rn_proximal_fun_g", "rn_compute_fixed_point_residual", "rn_dual_update"):
        getattr(lib, f).argtypes = [vp]
    lib.rn_update_primal_infeasibility.argtypes = [vp, dp]
    lib.rn_get_prox_distances.argtypes = [vp, dp, dp]
    lib.rn_buffer_size.argtypes = [vp, ip]
    lib.rn_buffer_size.restype = C.c_size_t
    lib.rn_get.argtypes = [vp, ip, dp, C.c_size_t]
    lib.rn_set.argtypes = [vp, ip, dp, C.c_size_t]
    lib.rn_get_operator.argtypes = [vp, ip, ip, dp, C.c_size_t]
    lib.rn_get_range.argtypes = [vp, ip, C.c_size_t, C.c_size_t, dp]
    lib.rn_set_range.argtypes = [vp, ip, C.c_size_t, C.c_size_t, dp]
    lib.rn_device_pointer.argtypes = [vp, ip, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    lib.rn_profile_enable.argtypes = [vp, ip]
    lib.rn_profile_reset.argtypes = [vp]
    lib.rn_profile_read.argtypes = [vp, dp, dp]
    lib.rn_algorithmic_bytes.argtypes = [vp, dp, dp]
    lib.rn_stream.argtypes = [vp]
    lib.rn_stream.restype = vp
    lib.rn_comm_unique_id.argtypes = [dp]
    lib.rn_comm_init.argtypes = [vp, ip, ip, dp]
    lib.rn_comm_init_timeout.argtypes = [vp, ip, ip, dp, C.c_double]
    lib.rn_comm_check.argtypes = [vp]
    lib.rn_comm_library.argtypes = [C.c_char_p, C.c_size_t]
    lib.rn_set_cut_stage.argtypes = [vp, ip]
    lib.rn_get_history_parts.argtypes = [vp, ip, ip, dp]
    lib.rn_get_counters.argtypes = [vp, dp]
    lib.rn_get_kernel_info.argtypes = [vp, dp]
    lib.rn_set_cut_children_moments.argtypes = [vp, dp, dp, C.c_size_t]
    lib.rn_set_operator_mode.argtypes = [vp, ip]
    lib.rn_get_operator_mode.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.rn_set_operator_storage.argtypes = [vp, ip]
    lib.rn_get_operator_storage.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.rn_set_sweep_pairing.argtypes = [vp, ip]
    lib.rn_get_sweep_pairing.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.rn_set_operator.argtypes = [vp, ip, ip, dp, C.c_size_t]
    lib.rn_set_operators.argtypes = [vp, C.c_size_t, dp, dp, dp, dp]
    lib.rn_get_operators.argtypes = [vp, C.c_size_t, dp, dp, dp, dp]
    lib.rn_set_operators_device.argtypes = [vp, C.c_size_t, ip, vp, vp, vp, vp]
    lib.rn_get_operators_device.argtypes = [vp, C.c_size_t, ip, vp, vp, vp, vp]
    lib.rn_set_warm_start.argtypes = [vp, ip]
    lib.rn_set_exchange_mode.argtypes = [vp, ip]
    lib.rn_debug_sweep_phase.argtypes = [vp, ip]
    lib.rn_debug_cut_buffer.argtypes = [vp, ip, dp, C.c_size_t]
    lib.rn_measure_hbm.argtypes = [vp, C.c_size_t, ip, dp, dp]
    lib.rn_set_algorithm.argtypes = [vp, ip, ip]
    for f in ("rn_fbe_reset", "rn_compute_hessian_oracle", "rn_compute_gradient_fbe", "rn_update_fixed_point_residual_nama",
              "rn_compute_lbfgs_direction", "rn_update_lbfgs_buffer", "rn_two_loop_recursion_lbfgs"):
        getattr(lib, f).argtypes = [vp]
    lib.rn_algorithm_fbe_nama.argtypes = [vp, ip, dp, dp, dp]
    lib.rn_compute_value_fbe.argtypes = [vp, dp]
    lib.rn_line_search_lbfgs_update.argtypes = [vp, C.c_double, dp]
    lib.rn_line_search_ame_lbfgs_update.argtypes = [vp, C.c_double, dp]
    lib.rn_lbfgs_state.argtypes = [vp, ip, dp, dp, dp, dp]
    lib.rn_lbfgs_column.argtypes = [vp, ip, ip, ip, dp, C.c_size_t]
    lib.rn_default_cut_stage.argtypes = [C.POINTER(RnDims), C.POINTER(RnTree)]
    lib.rn_partition_create.argtypes = [C.POINTER(RnDims), C.POINTER(RnTree), dp, dp, ip, ip, ip, C.POINTER(RnPartition)]
    lib.rn_partition_destroy.argtypes = [C.POINTER(RnPartition)]
    lib.rn_partition_destroy.restype = None
    lib.rn_create_sharded.argtypes = [C.POINTER(RnDims), C.POINTER(RnTree), dp, dp, ip, ip, ip, ip, ip, dp, C.POINTER(vp)]
    lib.rn_shard_info.argtypes = [vp, dp]
    lib.rn_shard_global_nodes.argtypes = [vp, dp, C.c_size_t]
    lib.rn_debug_set_allreduce.argtypes = [vp, ALLREDUCE_FN, vp]
    lib.rn_debug_local_group_create.argtypes = [ip, C.POINTER(vp)]
    lib.rn_debug_local_group_join.argtypes = [vp, vp, ip]
    lib.rn_debug_local_group_destroy.argtypes = [vp]
    lib.rn_guard_check.argtypes = [vp, dp]
    lib.rn_device_memory_info.argtypes = [vp, dp]
    lib.rn_reserve_iterations.argtypes = [vp, ip]
    lib.rn_debug_inject_allocation.argtypes = [vp, C.c_size_t]
    lib.rn_guard_report.argtypes = [dp]
    lib.rn_debug_guard_poke.argtypes = [vp, ip]
    lib.rn_fbe_counters.argtypes = [vp, dp]
    lib.rn_peer_inbox_create.argtypes = [vp, dp]
    lib.rn_peer_inbox_connect.argtypes = [vp, dp, ip]
    lib.rn_debug_peer_inbox_connect_local.argtypes = [C.POINTER(vp), ip]
    lib.rn_debug_peer_seq.argtypes = [vp, C.c_uint]
    lib.rn_set_exchange_transport.argtypes = [vp, ip]
    lib.rn_exchange_autotune.argtypes = [vp, ip, dp]
    lib.rn_set_fused_walk_dual.argtypes = [vp, ip]
    lib.rn_debug_set_knob.argtypes = [vp, ip, ip]
    lib.rn_debug_stream_info.argtypes = [vp, dp]
    lib.rn_debug_stream_live.argtypes = [vp, dp]
    lib.rn_debug_stream_units.argtypes = [vp, dp]
    lib.rn_debug_stream_product.argtypes = [vp, C.c_int, dp, dp, dp]
    lib.rn_debug_slab_product.argtypes = [vp, vp, vp]
    lib.rn_debug_dual_update.argtypes = [vp, vp, vp]
    lib.rn_profile_read_collective.argtypes = [vp, dp, dp]
    lib.rn_set_tree_data.argtypes = [vp, C.c_size_t, dp, dp, dp]
    lib.rn_set_tree_data_device.argtypes = [vp, C.c_size_t, ip, vp, vp, vp]
    lib.rn_get_tree_data.argtypes = [vp, C.c_size_t, dp, dp, dp]
    lib.rn_set_bounds.argtypes = [vp, ip, C.c_size_t, dp, dp, dp, dp, dp]
    lib.rn_set_bounds_device.argtypes = [vp, ip, C.c_size_t, ip, vp, vp, vp, vp, vp]
    lib.rn_get_bounds_layout.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    lib.rn_get_bounds.argtypes = [vp, C.c_size_t, dp, dp, dp, dp, dp]
    lib.rn_debug_cut_moments.argtypes = [vp, dp, dp, C.c_size_t]
    lib.rn_plan_report.argtypes = [vp, C.c_size_t, dp]
    lib.rn_plan_report_scenarios.argtypes = [vp, C.c_size_t, dp, dp]
    lib.rn_plan_report_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.rn_plan_quantiles.argtypes = [vp, ip, C.c_size_t, dp, C.c_size_t, dp]
    lib.rn_plan_quantiles_device.argtypes = [vp, ip, C.c_size_t, dp, C.POINTER(vp)]
    lib.rn_plan_paths.argtypes = [vp, ip, C.c_size_t, dp, dp]
    lib.rn_shift_warm_start.argtypes = [vp, ip]
    lib.rn_set_shift_map.argtypes = [vp, C.c_size_t, dp]
    lib.rn_get_shift_map.argtypes = [vp, ip, C.c_size_t, dp]
    lib.rn_estimate_lipschitz.argtypes = [vp, ip, C.c_double, ip, dp, dp, C.c_ulonglong, dp, dp]
    lib.rn_get_lipschitz.argtypes = [vp, dp, C.POINTER(C.c_int)]
    lib.rn_solve_certificate.argtypes = [vp, dp]
    lib.rn_solve_certificate_device.argtypes = [vp, C.POINTER(C.c_void_p)]
    lib.rn_debug_certificate_hz.argtypes = [vp, dp, dp]
    lib.rn_set_step_rule.argtypes = [vp, ip, C.c_double, ip]
    lib.rn_get_step_rule.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    _LIB = lib
    return lib


class RapidNetError(RuntimeError):
    pass


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel().astype(np.int32))


def _s(d, k):
    v = d[k]
    return v[0] if isinstance(v, (list, tuple, np.ndarray)) else v


class Solver:
    """Python mirror of the reference's Engine + SmpcController pair for one (network, tree, config) triple.

    Method names follow the reference (Engine.cuh:74-93, SmpcController.cuh:57-203); every method is one call
    through the C-ABI.  `problem` dicts use the reference's JSON schema.
    """

    def __init__(self, network, tree, config, precision="f64", device=0, structured=False, rank=0, nranks=1, cut_stage=0,
                 unique_id=None, knobs=None, operator_mode=None, operator_storage="native", sweep_pairing="auto", stop_tolerance=0.0,
                 stop_check_every=0, restart="off", step_rule=None):
        """nranks > 1: `tree` is the FULL scenario tree and the context is rank `rank`'s shard of it (rn_create_sharded:
        partition, communicator from `unique_id` -- None = none, the exchange is a test's job --, cut stage, children
        moments); self.nodes is then the LOCAL node count and self.global_nodes maps local -> full-tree node ids.
        operator_mode: "dense" | "structured" | "auto" (rn_set_operator_mode); None: `structured` decides between the first two --
        the tests and bench.py always say which storage they measure; the C-ABI's own default is auto.
        operator_storage: "native" | "f32" (rn_set_operator_storage): the element type of the dense blocks; "f32" on an f64 context
        streams half the bytes and accumulates in fp64.
        sweep_pairing: "auto" | "on" | "off" (rn_set_sweep_pairing): NAMA's two Hessian sweeps in one pass over the dense blocks; "on" adds
        fp32-stored blocks to what "auto" pairs.
        stop_tolerance, stop_check_every (rn_set_stop_tolerance): with a tolerance > 0 controlAction and algorithmApg end once the residual of
        the last iteration of a batch of stop_check_every iterations (0: the library's default, 20) is <= stop_tolerance; 0: fixed count.
        restart: "off" | "gradient" (rn_set_restart): the gradient test at every batch end restarts the momentum of apg_solve, algorithmApg and
        controlAction."""
        self.lib = load()
        self.structured = bool(structured)
        self.network, self.tree, self.config = network, tree, config
        self.nx, self.nu, self.nd = (int(_s(network, k)) for k in ("nx", "nu", "nd"))
        self.nv = int(_s(config, "nv"))
        self.N, self.K, self.nodes = (int(_s(tree, k)) for k in ("N", "K", "nodes"))
        self.ny = 2 * self.nx + self.nu
        self.max_iterations = int(_s(config, "maxIterations"))
        dims, t, keep = tree_structs(tree, self.nx, self.nu, self.nv, self.nd)
        ed, ep = _f64(tree["errorDemandNode"]), _f64(tree["errorPriceNode"])
        h = C.c_void_p()
        prec = RN_F64 if precision == "f64" else RN_F32
        self.rank, self.nranks = int(rank), int(nranks)
        if self.nranks > 1:
            idbuf = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
            rc = self.lib.rn_create_sharded(C.byref(dims), C.byref(t), ed.ctypes.data, ep.ctypes.data, prec, int(device), self.rank, self.nranks,
                                            int(cut_stage), C.cast(idbuf, C.c_void_p) if idbuf is not None else None, C.byref(h))
            if rc != 0:
                raise RapidNetError("rn_create_sharded failed (%d): %s" % (rc, self.lib.rn_last_error(None).decode()))
            self.h = h
            info = self.shardInfo()
            self.full_nodes, self.nodes = self.nodes, info["local_nodes"]
            self.global_nodes = self.shardGlobalNodes()
        else:
            rc = self.lib.rn_create(C.byref(dims), C.byref(t), prec, int(device), C.byref(h))
            if rc != 0:
                raise RapidNetError("rn_create failed (%d): %s" % (rc, self.lib.rn_last_error(None).decode()))
            self.h = h
            self._check(self.lib.rn_set_tree_errors(self.h, ed.ctypes.data, ep.ctypes.data))
        self._check(self.lib.rn_set_parameters(self.h, float(_s(config, "stepSize")), float(_s(config, "penaltyStateX")),
                                               float(_s(config, "penaltySafetyX"))))
        mode = OPS_MODES[operator_mode] if operator_mode is not None else (OPS_STRUCTURED if self.structured else OPS_DENSE)
        self._check(self.lib.rn_set_operator_mode(self.h, mode))
        self.structured = mode != OPS_DENSE
        if operator_storage != "native":      # (a context that never asks for it makes exactly the calls it always made)
            self._check(self.lib.rn_set_operator_storage(self.h, STORAGES[operator_storage]))
        if sweep_pairing != "auto":
            self._check(self.lib.rn_set_sweep_pairing(self.h, PAIRINGS[sweep_pairing]))
        if stop_tolerance or stop_check_every:      # (a context that never asks for it makes exactly the calls it always made)
            self.setStopTolerance(stop_tolerance, stop_check_every)
        if restart != "off":
            self.setRestart(restart)
        if step_rule is not None:      # ("lipschitz", or a tuple (rule, margin, iterations); a context that never asks makes no call)
            self.setStepRule(*((step_rule,) if isinstance(step_rule, str) else tuple(step_rule)))
        for k, v in (knobs or {}).items():
            self.debugSetKnob(k, v)

    def close(self):
        if getattr(self, "h", None):
            self.lib.rn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RapidNetError("rapidnet error %d: %s" % (rc, self.lib.rn_last_error(self.h).decode()))

    # ---- Engine -------------------------------------------------------------------------------------------
    def factorStep(self):
        n, c = self.network, self.config
        arrs = [_f64(n["matB"]), _f64(n["matGd"]), _f64(c["matL"]), _f64(c["matLhat"]), _f64(c["costW"]),
                _f64(c["matDiagPrecnd"]), _f64(n["vecXmin"]), _f64(n["vecXmax"]), _f64(n["vecXsafe"]), _f64(n["vecUmin"]),
                _f64(n["vecUmax"]), _f64(n["costAlpha1"])]
        assert arrs[0].size == self.nx * self.nu and arrs[2].size == self.nu * self.nv and arrs[3].size == self.nu * self.nd
        assert arrs[4].size == self.nu * self.nu and arrs[5].size == self.N * (2 * self.nx + self.nu)
        s = RnSystem(*[a.ctypes.data for a in arrs])
        self._check(self.lib.rn_factor_step(self.h, C.byref(s)))

    def updateStateControl(self, currentX=None, prevU=None, prevDemand=None):
        c = self.config
        a = [_f64(c["currentX"] if currentX is None else currentX), _f64(c["prevU"] if prevU is None else prevU),
             _f64(c["prevDemand"] if prevDemand is None else prevDemand)]
        assert a[0].size == self.nx and a[1].size == self.nu and a[2].size == self.nd
        self._check(self.lib.rn_update_state_control(self.h, *[v.ctypes.data for v in a]))

    def eliminateInputDistubanceCoupling(self, nominalDemand, nominalPrices):
        dh, ah = _f64(nominalDemand), _f64(nominalPrices)
        assert dh.size == self.N * self.nd and ah.size == self.N * self.nu
        self._check(self.lib.rn_eliminate_input_disturbance_coupling(self.h, dh.ctypes.data, ah.ctypes.data))

    def setUncertainty(self, demand=True, price=True, weightEconomical=1.0):
        self._check(self.lib.rn_set_uncertainty(self.h, int(demand), int(price), float(weightEconomical)))

    def initialiseSmpcController(self, nominalDemand, nominalPrices):
        """SmpcController::initialiseSmpcController, SmpcController.cu:476-487."""
        self.factorStep()
        self.updateStateControl()
        self.eliminateInputDistubanceCoupling(nominalDemand, nominalPrices)

    # ---- SmpcController -------------------------------------------------------------------------------------
    def apgReset(self):
        self._check(self.lib.rn_apg_reset(self.h))

    def apgIterate(self, n, history=True):
        hist = np.zeros(max(n, 1)) if history else None
        self._check(self.lib.rn_apg_iterate(self.h, int(n), hist.ctypes.data if history else None))
        return hist[:n] if history else None

    def algorithmApg(self, maxIterations=None):
        n = self.max_iterations if maxIterations is None else int(maxIterations)
        hist = np.zeros(max(n, 1))
        self._check(self.lib.rn_algorithm_apg(self.h, n, hist.ctypes.data))
        if getattr(self, "_stop_tol", 0.0) > 0:      # under a stop tolerance only the iterations that ran have an entry
            n = self.last_solve()["iterations"]
        return hist[:n]

    def apg_solve(self, maxIterations=None, tol=0.0, check_every=0, history=True):
        """rn_apg_solve: apgReset, then batches of check_every iterations (0: the library's default) until the residual of a batch's last
        iteration is <= tol (0: never) or maxIterations have run.  Returns (iterations run, vecPrimalInfs of those iterations or None)."""
        n = self.max_iterations if maxIterations is None else int(maxIterations)
        hist = np.zeros(max(n, 1)) if history else None
        run = C.c_int(0)
        self._check(self.lib.rn_apg_solve(self.h, n, float(tol), int(check_every), C.byref(run), hist.ctypes.data if history else None))
        return run.value, (hist[: run.value] if history else None)

    def setStopTolerance(self, tol, check_every=0):
        self._check(self.lib.rn_set_stop_tolerance(self.h, float(tol), int(check_every)))
        self._stop_tol = float(tol)

    def stopTolerance(self):
        """(tol, check_every) as set by setStopTolerance (0: off, the library's default batch length)"""
        t, e = C.c_double(0), C.c_int(0)
        self._check(self.lib.rn_get_stop_tolerance(self.h, C.byref(t), C.byref(e)))
        return t.value, e.value

    def setRestart(self, mode):
        """rn_set_restart: "off" | "gradient" (or the RN_RESTART_* value)"""
        self._check(self.lib.rn_set_restart(self.h, RESTARTS[mode] if isinstance(mode, str) else int(mode)))

    def restart(self):
        m = C.c_int(0)
        self._check(self.lib.rn_get_restart(self.h, C.byref(m)))
        return {v: k for k, v in RESTARTS.items()}[m.value]

    def last_restarts(self):
        """rn_get_restart_info: dict(restarts, last_at, tested, g, na2, nb2) of the last apg_solve / algorithmApg / controlAction"""
        cnt, last = np.zeros(4, dtype=np.int64), np.zeros(3)
        self._check(self.lib.rn_get_restart_info(self.h, cnt.ctypes.data, last.ctypes.data))
        return dict(restarts=int(cnt[0]), last_at=int(cnt[1]), tested=int(cnt[2]), g=float(last[0]), na2=float(last[1]), nb2=float(last[2]))

    def debugRestartTest(self):
        """rn_debug_restart_test (include/rapidnet_debug.h): (g, na2, nb2) of the gradient restart test on the current w, y+, y"""
        out = np.zeros(3)
        self._check(self.lib.rn_debug_restart_test(self.h, out.ctypes.data))
        return tuple(float(v) for v in out)

    def last_solve(self):
        """rn_get_last_solve: dict(iterations, stopped, first_below, batches) of the last apg_solve / algorithmApg / controlAction"""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rn_get_last_solve(self.h, out.ctypes.data))
        return dict(zip(("iterations", "stopped", "first_below", "batches"), (int(v) for v in out)))

    def controlAction(self, nominalDemand, nominalPrices, currentX=None, prevU=None, prevDemand=None, maxIterations=None,
                      project=False):
        c = self.config
        a = [_f64(c["currentX"] if currentX is None else currentX), _f64(c["prevU"] if prevU is None else prevU),
             _f64(c["prevDemand"] if prevDemand is None else prevDemand), _f64(nominalDemand), _f64(nominalPrices)]
        u0 = np.zeros(self.nu)
        n = self.max_iterations if maxIterations is None else int(maxIterations)
        self._check(self.lib.rn_control_action(self.h, *[v.ctypes.data for v in a], n, int(project), u0.ctypes.data))
        return u0

    def setExchangeMode(self, optimistic=True):
        """False / 0: exact, True / 1: optimistic batches (default) (include/rapidnet.h, rn_set_exchange_mode)."""
        self._check(self.lib.rn_set_exchange_mode(self.h, int(optimistic)))

    def setWarmStart(self, on=True):
        self._check(self.lib.rn_set_warm_start(self.h, int(on)))

    # ---- the warm start shifted one stage toward the root (rn_shift_warm_start ...) --------------------------------
    def shiftWarmStart(self, root_child=-1):
        """rn_shift_warm_start: y and y+ become the duals of the last solve moved one stage toward the root along child number root_child of
        the root (-1: its most probable child under the probabilities in force).  Between two control steps; it does not switch the warm
        start on (setWarmStart).  On a shard every rank calls it."""
        self._check(self.lib.rn_shift_warm_start(self.h, int(root_child)))

    def setShiftMap(self, node_map=None):
        """rn_set_shift_map: a correspondence of one's own, an entry per node of the WHOLE tree (a node, or -1 for "from zero"); None: the
        built-in rule again"""
        if node_map is None:
            self._check(self.lib.rn_set_shift_map(self.h, 0, None))
            return
        m = _i32(node_map)
        self._check(self.lib.rn_set_shift_map(self.h, m.size, m.ctypes.data))

    def getShiftMap(self, root_child=-1):
        """rn_get_shift_map: the correspondence in force (the caller's, or the built-in rule's for root_child), [nodes of the whole tree]"""
        m = np.zeros(self._treeNodes(), dtype=np.int32)
        self._check(self.lib.rn_get_shift_map(self.h, int(root_child), m.size, m.ctypes.data))
        return m

    # ---- the dual Lipschitz constant and the step size from it (rn_estimate_lipschitz ...) -----------------------------
    def estimateLipschitz(self, max_iterations=40, tol=0.0, check_every=0, start=None, seed=0, history=False):
        """rn_estimate_lipschitz: power iteration over the context's Hessian sweep.  start: None (the library's hashed start of `seed`) or
        (xi [nodes, 2nx], psi [nodes, nu]) in the layout of set(BUF_XI / BUF_PSI).  Returns dict(norm, rayleigh, residual, iterations) of the last
        record -- norm is the estimate, a lower bound of lambda_max -- and, with history, "history": [iterations run, 3].  On a shard every
        rank calls it."""
        n = int(max_iterations)
        out = np.zeros(len(LIP_COLUMNS))
        hist = np.zeros((max(n, 1), 3)) if history else None
        xi = psi = None
        if start is not None:
            xi, psi = _f64(start[0]), _f64(start[1])
            assert xi.size == self.nodes * 2 * self.nx and psi.size == self.nodes * self.nu
        self._check(self.lib.rn_estimate_lipschitz(self.h, n, float(tol), int(check_every), xi.ctypes.data if xi is not None else None,
                                                   psi.ctypes.data if psi is not None else None, int(seed), out.ctypes.data,
                                                   hist.ctypes.data if history else None))
        r = dict(zip(LIP_COLUMNS, (float(v) for v in out)))
        r["iterations"] = int(r["iterations"])
        if history:
            r["history"] = hist[: r["iterations"]]
        return r

    def lipschitz(self):
        """rn_get_lipschitz: the record held plus "stale" (the operators have changed since: factor step, own blocks, probabilities)"""
        out, stale = np.zeros(len(LIP_COLUMNS)), C.c_int(0)
        self._check(self.lib.rn_get_lipschitz(self.h, out.ctypes.data, C.byref(stale)))
        r = dict(zip(LIP_COLUMNS, (float(v) for v in out)))
        r["iterations"] = int(r["iterations"])
        r["stale"] = bool(stale.value)
        return r

    def setStepRule(self, rule="lipschitz", margin=0.9, iterations=0):
        """rn_set_step_rule: "fixed" (stepSize as configured) | "lipschitz" (the solves run with margin / norm, estimated on entry when
        no estimate is held or it is stale; iterations <= 0: 40)"""
        self._check(self.lib.rn_set_step_rule(self.h, STEP_RULES[rule] if isinstance(rule, str) else int(rule), float(margin), int(iterations)))

    def stepRule(self):
        """rn_get_step_rule: dict(rule, margin, iterations, step_size_in_force)"""
        r, m, i, s = C.c_int(0), C.c_double(0), C.c_int(0), C.c_double(0)
        self._check(self.lib.rn_get_step_rule(self.h, C.byref(r), C.byref(m), C.byref(i), C.byref(s)))
        return dict(rule={v: k for k, v in STEP_RULES.items()}[r.value], margin=m.value, iterations=i.value, step_size_in_force=s.value)

    def dualExtrapolationStep(self, lam):
        self._check(self.lib.rn_dual_extrapolation_step(self.h, float(lam)))

    def solveStep(self):
        self._check(self.lib.rn_solve_step(self.h))

    def proximalFunG(self):
        self._check(self.lib.rn_proximal_fun_g(self.h))

    def computeFixedPointResidual(self):
        self._check(self.lib.rn_compute_fixed_point_residual(self.h))

    def dualUpdate(self):
        self._check(self.lib.rn_dual_update(self.h))

    def updatePrimalInfeasibity(self):
        v = C.c_double(0)
        self._check(self.lib.rn_update_primal_infeasibility(self.h, C.byref(v)))
        return v.value

    def proxDistances(self):
        a, b = C.c_double(0), C.c_double(0)
        self._check(self.lib.rn_get_prox_distances(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- global FBE / NAMA (SmpcController.cu:884-1476, 1529-1586) ---------------------------------------------
    def setAlgorithm(self, name, lbfgsBufferSize=None):
        if lbfgsBufferSize is None:
            lbfgsBufferSize = int(_s(self.config, "lbfgsBufferSize")) if "lbfgsBufferSize" in self.config else 5
        self.algorithm = ALGORITHMS[name] if isinstance(name, str) else int(name)
        self.lbfgsBufferSize = int(lbfgsBufferSize)
        self._check(self.lib.rn_set_algorithm(self.h, self.algorithm, self.lbfgsBufferSize))

    def fbeReset(self):
        self._check(self.lib.rn_fbe_reset(self.h))

    def _algorithmFbeNama(self, maxIterations):
        n = self.max_iterations if maxIterations is None else int(maxIterations)
        hist, val, tau = (np.zeros(max(n, 1)) for _ in range(3))
        self._check(self.lib.rn_algorithm_fbe_nama(self.h, n, hist.ctypes.data, val.ctypes.data, tau.ctypes.data))
        return hist[:n], val[: max(n - 1, 0)], tau[: max(n - 1, 0)]

    def algorithmGlobalFbe(self, maxIterations=None):
        """returns (vecPrimalInfs, vecValueFbe, vecTau)"""
        assert getattr(self, "algorithm", ALG_APG) == ALG_GLOBAL_FBE
        return self._algorithmFbeNama(maxIterations)

    def algorithmNama(self, maxIterations=None):
        assert getattr(self, "algorithm", ALG_APG) == ALG_NAMA
        return self._algorithmFbeNama(maxIterations)

    def computeHessianOracalGlobalFbe(self):
        self._check(self.lib.rn_compute_hessian_oracle(self.h))

    def computeGradientFbe(self):
        self._check(self.lib.rn_compute_gradient_fbe(self.h))

    def updateFixedPointResidualNamaAlgorithm(self):
        self._check(self.lib.rn_update_fixed_point_residual_nama(self.h))

    def computeLbfgsDirection(self):
        self._check(self.lib.rn_compute_lbfgs_direction(self.h))

    def computeValueFbe(self):
        v = C.c_double(0)
        self._check(self.lib.rn_compute_value_fbe(self.h, C.byref(v)))
        return v.value

    def computeLineSearchLbfgsUpdate(self, valueFbeY):
        t = C.c_double(0)
        self._check(self.lib.rn_line_search_lbfgs_update(self.h, float(valueFbeY), C.byref(t)))
        return t.value

    def computeLineSearchAmeLbfgsUpdate(self, valueAmeY):
        t = C.c_double(0)
        self._check(self.lib.rn_line_search_ame_lbfgs_update(self.h, float(valueAmeY), C.byref(t)))
        return t.value

    def fbeCounters(self):
        """dict(searches, batches, sequential, sweep_pairs): how the line searches of the FBE / NAMA loops ran, and how many NAMA
        iterations ran their two Hessian sweeps in one pass over the operator blocks"""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rn_fbe_counters(self.h, out.ctypes.data))
        return dict(zip(("searches", "batches", "sequential", "sweep_pairs"), (int(v) for v in out)))

    def lbfgsState(self, col=None, mem=None, H=None, rho=None):
        """get (no arguments) or set lbfgsBufferCol / Memory / Hessian / Rho; returns (col, mem, H, rho[size+1])."""
        c, m, h = C.c_int(0 if col is None else col), C.c_int(0 if mem is None else mem), C.c_double(0 if H is None else H)
        r = np.zeros(self.lbfgsBufferSize + 1)
        if rho is not None:
            r[:] = rho
        self._check(self.lib.rn_lbfgs_state(self.h, 0 if col is None else 1, C.addressof(c), C.addressof(m), C.addressof(h),
                                            r.ctypes.data))
        return c.value, m.value, h.value, r

    def lbfgsColumn(self, which, col, values=None):
        """column `col` of matS (which=0) / matY (which=1) in the reference's (all xi | all psi) order."""
        n = self.nodes * (2 * self.nx + self.nu)
        a = np.zeros(n) if values is None else _f64(values).copy()
        assert a.size == n
        self._check(self.lib.rn_lbfgs_column(self.h, 0 if values is None else 1, int(which), int(col), a.ctypes.data, n))
        return a

    # ---- raw access -----------------------------------------------------------------------------------------
    def get(self, buf):
        n = self.lib.rn_buffer_size(self.h, buf)
        out = np.zeros(n)
        self._check(self.lib.rn_get(self.h, buf, out.ctypes.data, n))
        return out

    def set(self, buf, values):
        v = _f64(values)
        self._check(self.lib.rn_set(self.h, buf, v.ctypes.data, v.size))

    def getRange(self, buf, first, n):
        out = np.zeros(n)
        self._check(self.lib.rn_get_range(self.h, buf, int(first), int(n), out.ctypes.data))
        return out

    def setRange(self, buf, first, values):
        v = _f64(values)
        self._check(self.lib.rn_set_range(self.h, buf, int(first), v.size, v.ctypes.data))

    def getOperator(self, op, node):
        nx, nu, nv = self.nx, self.nu, self.nv
        n = {OP_PHI: nv * 2 * nx, OP_D: nv * 2 * nx, OP_PSI: nv * nu, OP_F: nv * nu, OP_OMEGA: nv * nv, OP_THETA: nv * nx,
             OP_G: nv * nx}[op]
        out = np.zeros(n)
        self._check(self.lib.rn_get_operator(self.h, op, int(node), out.ctypes.data, n))
        return out

    def setOperator(self, op, node, values):
        """hand in one node's block (OP_PHI, OP_PSI, OP_D, OP_F; col-major nv x (2nx | nu)); an auto context becomes dense"""
        v = _f64(values)
        self._check(self.lib.rn_set_operator(self.h, int(op), int(node), v.ctypes.data, v.size))

    def _opDims(self):
        return {"Phi": self.nv * 2 * self.nx, "Psi": self.nv * self.nu, "D": self.nv * 2 * self.nx, "Ftil": self.nv * self.nu}

    def setOperators(self, phi=None, psi=None, D=None, F=None):
        """rn_set_operators: every node's blocks at once from numpy arrays in the reference's layout ([nodes][2nx | nu columns][nv]); None: that
        operator stays as it is.  An auto context becomes dense."""
        dims = self._opDims()
        arrs = [None if v is None else _f64(v) for v in (phi, psi, D, F)]
        for a, nm in zip(arrs, ("Phi", "Psi", "D", "Ftil")):
            if a is not None and a.size != self.nodes * dims[nm]:
                raise ValueError("setOperators: %s needs %d x %d values, got %d" % (nm, self.nodes, dims[nm], a.size))
        self._check(self.lib.rn_set_operators(self.h, self.nodes, *[None if a is None else a.ctypes.data for a in arrs]))

    def getOperators(self, ops=("Phi", "Psi", "D", "Ftil")):
        """rn_get_operators: {name: [nodes][dim]} the stored blocks of the named operators (a context with dense blocks)"""
        dims = self._opDims()
        out = {nm: np.zeros((self.nodes, dims[nm])) for nm in ops}
        self._check(self.lib.rn_get_operators(self.h, self.nodes, *[out[nm].ctypes.data if nm in out else None for nm in ("Phi", "Psi", "D", "Ftil")]))
        return out

    def setOperatorsDevice(self, precision, phi=0, psi=0, D=0, F=0, nodes=None):
        """rn_set_operators_device: integer device addresses (0: not given) of arrays of `precision` ("f64" | "f32" or an RN_F* value)
        elements; one launch on the context's stream, nothing is waited for"""
        prec = {"f64": RN_F64, "f32": RN_F32}.get(precision, precision)
        self._check(self.lib.rn_set_operators_device(self.h, self.nodes if nodes is None else int(nodes), int(prec), *[int(p) or None for p in (phi, psi, D, F)]))

    def getOperatorsDevice(self, precision, phi=0, psi=0, D=0, F=0, nodes=None):
        """rn_get_operators_device: the stored blocks into the caller's device arrays (0: skipped); stream-ordered, not waited for"""
        prec = {"f64": RN_F64, "f32": RN_F32}.get(precision, precision)
        self._check(self.lib.rn_get_operators_device(self.h, self.nodes if nodes is None else int(nodes), int(prec), *[int(p) or None for p in (phi, psi, D, F)]))

    def operatorMode(self):
        """(requested, active) as "dense" | "structured" | "auto" """
        r, a = C.c_int(0), C.c_int(0)
        self._check(self.lib.rn_get_operator_mode(self.h, C.byref(r), C.byref(a)))
        names = {v: k for k, v in OPS_MODES.items()}
        return names[r.value], names[a.value]

    def operatorStorage(self):
        """(requested, active) as "native" | "f32": active is "f32" only while dense blocks exist in fp32"""
        r, a = C.c_int(0), C.c_int(0)
        self._check(self.lib.rn_get_operator_storage(self.h, C.byref(r), C.byref(a)))
        names = {v: k for k, v in STORAGES.items()}
        return names[r.value], names[a.value]

    def sweepPairing(self):
        """(requested as "auto" | "on" | "off", active): active is 1 when the context as it stands would pair its next NAMA line search"""
        r, a = C.c_int(0), C.c_int(0)
        self._check(self.lib.rn_get_sweep_pairing(self.h, C.byref(r), C.byref(a)))
        return {v: k for k, v in PAIRINGS.items()}[r.value], a.value

    # ---- scenario probabilities and tree errors in place (rn_set_tree_data ...) ------------------------------------
    def _treeNodes(self):
        """the node count a SET takes: the full tree's on a shard made by rn_create_sharded"""
        return self.full_nodes if self.nranks > 1 else self.nodes

    def setTreeData(self, prob=None, errorDemand=None, errorPrice=None):
        """rn_set_tree_data: new probNode [nodes], errorDemandNode [nodes][nd], errorPriceNode [nodes][nu] (None: that array stays as it is); on a
        shard (nranks > 1) the FULL tree's arrays.  With prob given the affine terms must be recomputed before the next iteration."""
        n = self._treeNodes()
        arrs = [None if v is None else _f64(v) for v in (prob, errorDemand, errorPrice)]
        for a, nm, dim in zip(arrs, ("prob", "errorDemand", "errorPrice"), (1, self.nd, self.nu)):
            if a is not None and a.size != n * dim:
                raise ValueError("setTreeData: %s needs %d x %d values, got %d" % (nm, n, dim, a.size))
        self._check(self.lib.rn_set_tree_data(self.h, n, *[None if a is None else a.ctypes.data for a in arrs]))

    def setTreeDataDevice(self, precision, prob=0, errorDemand=0, errorPrice=0, nodes=None):
        """rn_set_tree_data_device: integer device addresses (0: not given) of arrays of `precision` ("f64" | "f32" or an RN_F* value) elements;
        launches on the context's stream, nothing is waited for"""
        prec = {"f64": RN_F64, "f32": RN_F32}.get(precision, precision)
        self._check(self.lib.rn_set_tree_data_device(self.h, self._treeNodes() if nodes is None else int(nodes), int(prec),
                                                     *[int(p) or None for p in (prob, errorDemand, errorPrice)]))

    def getTreeData(self):
        """rn_get_tree_data: dict(prob [nodes], errorDemand [nodes][nd], errorPrice [nodes][nu]) as the context holds them (local rows on a shard)"""
        out = {"prob": np.zeros(self.nodes), "errorDemand": np.zeros((self.nodes, self.nd)), "errorPrice": np.zeros((self.nodes, self.nu))}
        self._check(self.lib.rn_get_tree_data(self.h, self.nodes, out["prob"].ctypes.data, out["errorDemand"].ctypes.data, out["errorPrice"].ctypes.data))
        return out

    # ---- box and safety bounds per stage or per node in place (rn_set_bounds ...) ----------------------------------
    def _boundsRows(self, granularity):
        g = BOUNDS.get(granularity, granularity)
        return int(g), {BOUNDS_SHARED: 1, BOUNDS_PER_STAGE: self.N, BOUNDS_PER_NODE: self.nodes}.get(g, 0)

    def setBounds(self, granularity, xmin=None, xmax=None, xsafe=None, umin=None, umax=None, rows=None):
        """rn_set_bounds: physical bounds, xmin / xmax / xsafe [rows][nx], umin / umax [rows][nu]; granularity "shared" | "stage" | "node" or a
        BOUNDS_* value (rows 1, N, the context's local node count); None keeps that array while the granularity stays what it is"""
        g, r = self._boundsRows(granularity)
        r = r if rows is None else int(rows)
        arrs = [None if v is None else _f64(v) for v in (xmin, xmax, xsafe, umin, umax)]
        for a, nm, dim in zip(arrs, ("xmin", "xmax", "xsafe", "umin", "umax"), (self.nx, self.nx, self.nx, self.nu, self.nu)):
            if a is not None and a.size != r * dim:
                raise ValueError("setBounds: %s needs %d x %d values, got %d" % (nm, r, dim, a.size))
        self._check(self.lib.rn_set_bounds(self.h, g, r, *[None if a is None else a.ctypes.data for a in arrs]))

    def setBoundsDevice(self, granularity, precision, xmin=0, xmax=0, xsafe=0, umin=0, umax=0, rows=None):
        """rn_set_bounds_device: integer device addresses (0: not given) of arrays of `precision` ("f64" | "f32" or an RN_F* value) elements;
        launches on the context's stream, nothing is waited for and the values are not validated"""
        g, r = self._boundsRows(granularity)
        prec = {"f64": RN_F64, "f32": RN_F32}.get(precision, precision)
        self._check(self.lib.rn_set_bounds_device(self.h, g, r if rows is None else int(rows), int(prec),
                                                  *[int(p) or None for p in (xmin, xmax, xsafe, umin, umax)]))

    def boundsLayout(self):
        """rn_get_bounds_layout: (granularity as a BOUNDS_* value, rows)"""
        g, r = C.c_int(0), C.c_size_t(0)
        self._check(self.lib.rn_get_bounds_layout(self.h, C.byref(g), C.byref(r)))
        return g.value, r.value

    def getBounds(self):
        """rn_get_bounds: dict(granularity, rows, xmin, xmax, xsafe [rows][nx], umin, umax [rows][nu]), physical values as the context holds them"""
        g, r = self.boundsLayout()
        out = {k: np.zeros((r, self.nx if k[0] == "x" else self.nu)) for k in ("xmin", "xmax", "xsafe", "umin", "umax")}
        self._check(self.lib.rn_get_bounds(self.h, r, *[out[k].ctypes.data for k in ("xmin", "xmax", "xsafe", "umin", "umax")]))
        out["granularity"], out["rows"] = g, r
        return out

    # ---- what the plan at hand costs and where it violates its bounds (rn_plan_report ...) ------------------------
    def planLeaves(self):
        """rows of the per-scenario table: the context's (local) node count at the last stage"""
        st = _i32(self.tree["stages"])
        mine = np.asarray(self.global_nodes) if self.nranks > 1 else np.arange(self.nodes)
        return int((st[mine] == st.max()).sum())

    def planReport(self):
        """rn_plan_report + rn_plan_report_scenarios: {"stage": {column: array [N]}, "scenario": {column: array [leaves]}, "leafNode": array
        [leaves] of (local) node indices}, columns as PLAN_COLUMNS.  On a shard every rank calls it (both calls are collective)."""
        nc, leaves = len(PLAN_COLUMNS), self.planLeaves()
        st, sc, ln = np.zeros((self.N, nc)), np.zeros((leaves, nc)), np.zeros(leaves, dtype=np.int32)
        self._check(self.lib.rn_plan_report(self.h, self.N, st.ctypes.data))
        self._check(self.lib.rn_plan_report_scenarios(self.h, leaves, sc.ctypes.data, ln.ctypes.data))
        return {"stage": {k: st[:, i].copy() for i, k in enumerate(PLAN_COLUMNS)}, "scenario": {k: sc[:, i].copy() for i, k in enumerate(PLAN_COLUMNS)},
                "leafNode": ln}

    def planReportDevice(self):
        """rn_plan_report_device: (address of the per-stage table, COLUMN-major [columns][N] doubles; address of the per-scenario table
        [leaves][columns] doubles; leaves), valid until the next report; nothing is waited for"""
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_size_t(0)
        self._check(self.lib.rn_plan_report_device(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    # ---- dual bound and optimality gap of the multiplier at hand (rn_solve_certificate ...) ------------------------
    def solveCertificate(self):
        """rn_solve_certificate: {column: value} for CERT_COLUMNS at y = (BUF_UPD_XI, BUF_UPD_PSI).  "dual" is a lower bound of the optimal
        value only with "valid" == 1; "gap" bounds the suboptimality of z(y) only with "uExcess" == 0.  One sweep plus two launches and one
        synchronisation; the solve continues as if the call had not happened.  BUF_CERT_X / BUF_CERT_U hold x(y), u(y) afterwards."""
        out = np.zeros(CERT_COLS)
        self._check(self.lib.rn_solve_certificate(self.h, out.ctypes.data))
        return dict(zip(CERT_COLUMNS, (float(v) for v in out)))

    def solveCertificateDevice(self):
        """rn_solve_certificate_device: the address of the record (CERT_COLS doubles, device memory), valid until the next certificate;
        nothing is waited for"""
        a = C.c_void_p()
        self._check(self.lib.rn_solve_certificate_device(self.h, C.byref(a)))
        return a.value

    def debugCertificateHz(self):
        """rn_debug_certificate_hz (include/rapidnet_debug.h): (Hz_xi [nodes * 2 nx], Hz_psi [nodes * nu]) of the last certificate's sweep"""
        a, b = np.zeros(self.nodes * 2 * self.nx), np.zeros(self.nodes * self.nu)
        self._check(self.lib.rn_debug_certificate_hz(self.h, a.ctypes.data, b.ctypes.data))
        return a, b

    # ---- what the plan at hand looks like across the tree (rn_plan_quantiles, rn_plan_paths) -----------------------
    def _band(self, which):
        w = BANDS.get(which, which)
        return int(w), {BAND_X: self.nx, BAND_U: self.nu}.get(w, 1)

    def bandLeaves(self):
        """rows of planPaths: the node count of the WHOLE tree's last stage (on a shard too)"""
        st = _i32(self.tree["stages"])
        return int((st == st.max()).sum())

    def planQuantiles(self, which, q):
        """rn_plan_quantiles: weighted quantiles of every component of x or u ("x" | "u" or a BAND_* value) per stage at the levels q (any
        order, at most BAND_MAX_LEVELS), an array [stages][dim][len(q)].  On a shard every rank calls it and receives the whole tree's."""
        w, dim = self._band(which)
        q = _f64(q)
        out = np.zeros((self.N, dim, max(q.size, 1)))
        self._check(self.lib.rn_plan_quantiles(self.h, w, q.size, q.ctypes.data, self.N, out.ctypes.data))
        return out

    def planQuantilesDevice(self, which, q):
        """rn_plan_quantiles_device: the address of the same table, [stages][dim][len(q)] doubles in device memory, valid until the next
        quantile call; nothing is waited for"""
        w, _ = self._band(which)
        q = _f64(q)
        a = C.c_void_p()
        self._check(self.lib.rn_plan_quantiles_device(self.h, w, q.size, q.ctypes.data, C.byref(a)))
        return a.value

    def planPaths(self, which):
        """rn_plan_paths: (array [leaves][N][dim]: the rows of x or u along the path of every leaf of the whole tree, root first; array [leaves]
        of the leaves' node indices in the whole tree).  On a shard every rank calls it."""
        w, dim = self._band(which)
        leaves = self.bandLeaves()
        out, ln = np.zeros((leaves, self.N, dim)), np.zeros(leaves, dtype=np.int32)
        self._check(self.lib.rn_plan_paths(self.h, w, leaves, out.ctypes.data, ln.ctypes.data))
        return out, ln

    def updateTree(self, tree):
        """a re-weighted scenario tree of the SAME topology (on a shard: the full tree): replaces self.tree and hands its probabilities and errors
        to the context (setTreeData with all three arrays)"""
        for k in ("N", "K", "nodes", "nNonLeafNodes"):
            if int(_s(tree, k)) != int(_s(self.tree, k)):
                raise ValueError("updateTree: %s differs from the context's tree" % k)
        for k in ("stages", "ancestor", "nChildren", "nodesPerStage"):
            if not np.array_equal(_i32(tree[k]), _i32(self.tree[k])):
                raise ValueError("updateTree: the topology (%s) differs from the context's tree" % k)
        self.tree = tree
        self.setTreeData(tree["probNode"], tree["errorDemandNode"], tree["errorPriceNode"])

    def debugCutMoments(self):
        """rn_debug_cut_moments: (E [parents][nd], P [parents]) as the context holds them"""
        n = self.shardInfo()["cut_parents"]
        E, P = np.zeros((n, self.nd)), np.zeros(n)
        self._check(self.lib.rn_debug_cut_moments(self.h, E.ctypes.data, P.ctypes.data, n))
        return E, P

    def synchronize(self):
        self._check(self.lib.rn_synchronize(self.h))

    # ---- measurement ----------------------------------------------------------------------------------------
    def profileEnable(self, on=1):
        self._check(self.lib.rn_profile_enable(self.h, int(on)))

    def profileReset(self):
        self._check(self.lib.rn_profile_reset(self.h))

    def profileRead(self):
        ms = np.zeros(4)
        n = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rn_profile_read(self.h, ms.ctypes.data, n.ctypes.data))
        return ms, n

    def profileReadCollective(self):
        """(ms, count) of the all-reduces timed since the last profileReset (sharded contexts; inside class 1 of profileRead)."""
        ms, n = C.c_double(0), C.c_long(0)
        self._check(self.lib.rn_profile_read_collective(self.h, C.addressof(ms), C.addressof(n)))
        return ms.value, n.value

    def guardCheck(self):
        """red-zone bytes overwritten so far (0 unless the context was created under RAPIDNET_GUARD=1)."""
        bad = C.c_long(0)
        self._check(self.lib.rn_guard_check(self.h, C.addressof(bad)))
        return bad.value

    def peerInboxCreate(self):
        """this rank's inbox for the one-shot exchange: returns its 64-byte IPC handle (bytes)"""
        buf = C.create_string_buffer(64)
        self._check(self.lib.rn_peer_inbox_create(self.h, C.cast(buf, C.c_void_p)))
        return bytes(buf.raw)

    def peerInboxConnect(self, handles):
        """handles: the 64-byte IPC handles of all ranks, in rank order"""
        blob = b"".join(bytes(h) for h in handles)
        buf = C.create_string_buffer(blob, len(blob))
        self._check(self.lib.rn_peer_inbox_connect(self.h, C.cast(buf, C.c_void_p), len(handles)))

    def debugPeerSeq(self, seq):
        self._check(self.lib.rn_debug_peer_seq(self.h, int(seq) & 0xFFFFFFFF))

    def setExchangeTransport(self, transport):
        """EXCHANGE_COLLECTIVE (0): the cut payload is all-reduced by the communicator; EXCHANGE_ONESHOT (1): one-shot peer writes (needs
        connected inboxes); EXCHANGE_AUTO (2, the default): the context times both in its first batch and keeps the faster"""
        self._check(self.lib.rn_set_exchange_transport(self.h, int(transport)))

    def exchangeAutotune(self, iterations=0):
        """rn_exchange_autotune: iterations > 0 tunes now (collective: every rank calls it), 0 reports the last result"""
        out = np.zeros(8)
        self._check(self.lib.rn_exchange_autotune(self.h, int(iterations), out.ctypes.data))
        return {"transport": int(out[0]), "candidates": int(out[1]), "collective_us": float(out[2]), "oneshot_us": float(out[3]),
                "own_collective_us": float(out[4]), "own_oneshot_us": float(out[5]), "iterations": int(out[6]), "tunes": int(out[7])}

    def setFusedWalkDual(self, on):
        """1 / 0: forward walk + dual update in one launch inside batches of >= 16 iterations (identical iterates) on / off; -1: by shape (default)"""
        self._check(self.lib.rn_set_fused_walk_dual(self.h, int(on)))

    def debugSetKnob(self, knob, value):
        """rn_debug_set_knob (include/rapidnet_debug.h): force a launch-shape choice the library otherwise makes by problem size; before factorStep.
        knob: a KNOB_* id or its name without the prefix ("dual_trips", "vlv_wide", ...); value -1: the library's own choice"""
        k = KNOBS[knob.lower()] if isinstance(knob, str) else int(knob)
        self._check(self.lib.rn_debug_set_knob(self.h, k, int(value)))

    def streamInfo(self):
        """rn_debug_stream_info (include/rapidnet_debug.h): what the launches of k_stream_gemv look like.  splitFirst: first node of the
        split last round (= nodes: not split; -1: the factor step has not decided yet), splitSpanHalf: the span the second workgroup of
        a split block starts at, twoPerCU: which instantiation runs, numCUs: the device's compute units (valid before the factor step)."""
        out = np.zeros(4, dtype=np.int32)
        self._check(self.lib.rn_debug_stream_info(self.h, out.ctypes.data))
        return dict(zip(("splitFirst", "splitSpanHalf", "twoPerCU", "numCUs"), (int(v) for v in out)))

    def streamLive(self):
        """rn_debug_stream_live (include/rapidnet_debug.h): what the most recent launch of k_stream_gemv walked, summed over the blocks."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rn_debug_stream_live(self.h, out.ctypes.data))
        return dict(zip(("liveSpans", "spans", "liveColumns", "columns"), (int(v) for v in out)))

    def streamUnits(self):
        """rn_debug_stream_units (include/rapidnet_debug.h): the most recent launch of k_stream_gemv in the units its skip walks -- half-spans
        where it skips them by themselves, whole spans elsewhere."""
        out = np.zeros(3, dtype=np.int64)
        self._check(self.lib.rn_debug_stream_units(self.h, out.ctypes.data))
        return dict(zip(("liveUnits", "units", "columnsPerUnit"), (int(v) for v in out)))

    def streamProduct(self, pair=False):
        """rn_debug_stream_product (include/rapidnet_debug.h): k_stream_gemv alone at the accelerated dual (BUF_ACC_*), as a sweep of this context
        would launch it.  Returns {"my": [nodes][2 nv]}; on a context with a split last round also "my2": [nodes - splitFirst][2 nv], the second
        workgroups' partials ("my" then holds the first workgroups' for those blocks); pair=True: one launch with y (BUF_XI / BUF_PSI) as the
        second right-hand side, its product in "myB" (unsplit: no "my2")."""
        rows = 2 * self.nv
        out = {"my": np.zeros((self.nodes, rows))}
        first = self.streamInfo()["splitFirst"]
        if pair:
            out["myB"] = np.zeros((self.nodes, rows))
        elif 0 <= first < self.nodes:
            out["my2"] = np.zeros((self.nodes - first, rows))
        self._check(self.lib.rn_debug_stream_product(self.h, int(bool(pair)), out["my"].ctypes.data, out["my2"].ctypes.data if "my2" in out else None,
                                                     out["myB"].ctypes.data if pair else None))
        return out

    SLAB_LAUNCHES = {"pair": 0, "comp": 1, "prep_m2": 2, "single": 3}
    SLAB_KERNELS = {0: None, 1: "k_gemm_vlv", 2: "k_gemm_vlv_wide", 3: "k_gemm_comp", 4: "k_gemm_prep_m2", 5: "k_gemm_slab", 6: "k_gemm_shared"}
    SLAB_INFO = ("kernel", "kernel2", "nw", "pipe", "frag", "ct", "grid", "lds", "m", "k", "kp", "ldin", "m2", "k2", "kp2", "ldin2", "nw2", "grid2", "lds2",
                 "auxSplit", "numCUs", "structPrep", "outNodes", "inOffset")

    def slabOutNodes(self):
        """Rows of the output buffers of slabProduct: the nodes, padded past every slab and every wide workgroup."""
        return ((self.nodes + 47) // 48 + 1) * 48

    def slabProduct(self, launch, MA, MB=None, inp=None, aux=None, aux2=None, prob=None, role=0, storeV=True, ldA=None, ldB=None, fill=0.0):
        """rn_debug_slab_product (include/rapidnet_debug.h): one launch step of the products with the shared operators, as a sweep of this context
        shapes it, over the caller's operators (MA, MB: m x k arrays) and operands (inp [nodes][k], aux, aux2, prob).  ldA / ldB: the row lengths of
        the two output buffers (None: that output does not exist); both are [slabOutNodes()][ld], pre-filled with `fill` and returned whole --
        whatever the launch did not write still holds it.  Returns (outA, outB, info), info a dict over SLAB_INFO with the kernels by name."""
        class _Args(C.Structure):
            _fields_ = [("launch", C.c_int), ("role", C.c_int), ("storeV", C.c_int)] + [(n, C.c_void_p) for n in ("MA", "MB", "in_", "aux", "aux2", "prob", "outA", "outB")] + \
                       [("nOutA", C.c_size_t), ("nOutB", C.c_size_t)]
        keep = []

        def _in(x, order="C"):
            if x is None:
                return None
            arr = np.require(np.asarray(x, dtype=np.float64), requirements=["F" if order == "F" else "C", "A"])
            keep.append(arr)
            return arr.ctypes.data
        on = self.slabOutNodes()
        outA = np.full((on, ldA), float(fill)) if ldA else None
        outB = np.full((on, ldB), float(fill)) if ldB else None
        args = _Args(self.SLAB_LAUNCHES[launch], int(role), int(bool(storeV)), _in(MA, "F"), _in(MB, "F"), _in(inp), _in(aux), _in(aux2), _in(prob),
                     outA.ctypes.data if ldA else None, outB.ctypes.data if ldB else None, outA.size if ldA else 0, outB.size if ldB else 0)
        info = np.zeros(24, dtype=np.int32)
        self._check(self.lib.rn_debug_slab_product(self.h, C.addressof(args), info.ctypes.data))
        d = dict(zip(self.SLAB_INFO, (int(v) for v in info)))
        d["kernel"], d["kernel2"] = self.SLAB_KERNELS[d["kernel"]], self.SLAB_KERNELS[d["kernel2"]]
        return outA, outB, d

    DUAL_FORMS = {"main": 0, "exact": 1, "exact_sharded": 2, "optimistic_close": 3, "info": 4, "next_w": 5}
    DUAL_INFO = ("lambda", "invLambda", "ln", "thrX", "thrS", "d2x", "d2s", "distX", "distS", "tripped", "scaleX", "scaleS", "violated", "absXi", "valXi", "idxXi",
                 "absPsi", "valPsi", "idxPsi", "hist", "kernel", "grid", "trips", "pipe", "crownBlocks", "bps", "vpn", "cs", "K", "node0", "eltBlocks", "fixBlocks",
                 "crownElems", "countCrown", "scale", "bStrideStage", "bStrideNode", "bRows", "preScale", "itAfter")

    def debugDualUpdate(self, form="main", materialize=False, flat=False, unscaled=False, iteration=0, fill=7777.0, tables=False):
        """rn_debug_dual_update (include/rapidnet_debug.h): the dual update of one iteration alone on the context's buffers as they stand (Hx =
        BUF_PRIMAL_*, w = BUF_ACC_*, y = BUF_UPD_*), through the batch loop's own launch steps.  Returns (out, info): out["ynew"], ["wnext"], ["z"],
        ["res"] are [nodes][ny] in the context's interleaved rows, pre-filled with `fill` (what was not written still holds it); out["partials"]
        [grid][8] the raw partials of the main pass; tables=True adds lo, hi [nodes][ny], sqrtp, dy [N][ny], blo, bhi [bRows][ny], stageOf.  info: a dict
        over DUAL_INFO (floats; "kernel" by name).  form "info" launches nothing (out holds the fills), "next_w" returns only out["wnext"]."""
        class _Args(C.Structure):
            _fields_ = [(n, C.c_int) for n in ("form", "materialize", "flat", "unscaled", "iteration")] + \
                       [(n, C.c_void_p) for n in ("ynew", "wnext", "z", "res", "lo", "hi", "sqrtp", "dy", "blo", "bhi", "stageOf", "partials")] + [("nPartials", C.c_size_t)]
        f = self.DUAL_FORMS[form]
        shape = (self.nodes, self.ny)
        info = np.zeros(len(self.DUAL_INFO))
        if form == "next_w":
            w = np.full(shape, float(fill))
            a = _Args(f, 0, 0, 0, int(iteration), None, w.ctypes.data, *([None] * 10), 0)
            self._check(self.lib.rn_debug_dual_update(self.h, C.addressof(a), info.ctypes.data))
            return {"wnext": w}, None
        a0 = _Args(self.DUAL_FORMS["info"], int(bool(materialize)), int(bool(flat)), int(bool(unscaled)), int(iteration), *([None] * 12), 0)
        self._check(self.lib.rn_debug_dual_update(self.h, C.addressof(a0), info.ctypes.data))
        d0 = dict(zip(self.DUAL_INFO, (float(v) for v in info)))
        out = {k: np.full(shape, float(fill)) for k in ("ynew", "wnext", "z", "res")}
        out["partials"] = np.full((int(d0["grid"]), 8), float(fill))
        if tables:
            out.update(lo=np.zeros(shape), hi=np.zeros(shape), sqrtp=np.zeros(self.nodes), dy=np.zeros((self.N, self.ny)), blo=np.zeros((int(d0["bRows"]), self.ny)),
                       bhi=np.zeros((int(d0["bRows"]), self.ny)), stageOf=np.zeros(self.nodes, dtype=np.int32))
        ptr = lambda k: out[k].ctypes.data if k in out else None
        a = _Args(f, int(bool(materialize)), int(bool(flat)), int(bool(unscaled)), int(iteration), ptr("ynew"), ptr("wnext"), ptr("z"), ptr("res"), ptr("lo"), ptr("hi"),
                  ptr("sqrtp"), ptr("dy"), ptr("blo"), ptr("bhi"), ptr("stageOf"), ptr("partials"), out["partials"].shape[0])
        self._check(self.lib.rn_debug_dual_update(self.h, C.addressof(a), info.ctypes.data))
        d = dict(zip(self.DUAL_INFO, (float(v) for v in info)))
        d["kernel"] = "k_dual_stage" if d["kernel"] == 1 else "k_dual_fused"
        return out, d

    def debugGuardPoke(self, nbytes):
        self._check(self.lib.rn_debug_guard_poke(self.h, int(nbytes)))

    def deviceMemoryInfo(self):
        out = (C.c_size_t * 4)()
        self._check(self.lib.rn_device_memory_info(self.h, C.addressof(out)))
        return dict(zip(("free", "total", "context_bytes", "live_contexts"), (int(v) for v in out)))

    def reserveIterations(self, n):
        self._check(self.lib.rn_reserve_iterations(self.h, int(n)))

    def measureHbm(self, nbytes=1 << 30, reps=3):
        """(read-only GB/s, copy GB/s) of do-nothing flat streaming kernels on this device."""
        r, c = C.c_double(0), C.c_double(0)
        self._check(self.lib.rn_measure_hbm(self.h, int(nbytes), int(reps), C.addressof(r), C.addressof(c)))
        return r.value, c.value

    def devicePointer(self, buffer_id):
        """(raw device address, element count, 'f64' | 'f32') of a buffer kept in the reference's node-major layout (X, U, V, UHAT, E,
        BETA, ALPHA, XDIR, UDIR): the counterpart of the reference's raw device getters; RapidNetError for the others (use get)."""
        p, n, prec = C.c_void_p(), C.c_size_t(0), C.c_int(0)
        self._check(self.lib.rn_device_pointer(self.h, int(buffer_id), C.byref(p), C.byref(n), C.byref(prec)))
        return p.value, n.value, "f64" if prec.value == RN_F64 else "f32"

    def algorithmicBytes(self):
        a, b = C.c_double(0), C.c_double(0)
        self._check(self.lib.rn_algorithmic_bytes(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- multi-GPU ------------------------------------------------------------------------------------------
    def commInit(self, rank, nranks, unique_id_bytes, timeout=None):
        """unique_id_bytes None: record rank / nranks only (tests emulate the exchange with debugCutBuffer).
        timeout (seconds; None: $RAPIDNET_COMM_TIMEOUT_S or 120): a rank whose peers do not arrive gets RapidNetError (RN_E_COMM)
        back instead of waiting for ever; the context stays usable without a communicator."""
        if unique_id_bytes is None:
            self._check(self.lib.rn_comm_init(self.h, int(rank), int(nranks), None))
            return
        buf = C.create_string_buffer(bytes(unique_id_bytes), 128)
        if timeout is None:
            self._check(self.lib.rn_comm_init(self.h, int(rank), int(nranks), C.cast(buf, C.c_void_p)))
        else:
            self._check(self.lib.rn_comm_init_timeout(self.h, int(rank), int(nranks), C.cast(buf, C.c_void_p), float(timeout)))

    def commCheck(self):
        self._check(self.lib.rn_comm_check(self.h))

    def debugSweepPhase(self, phase):
        self._check(self.lib.rn_debug_sweep_phase(self.h, int(phase)))

    def debugCutBuffer(self, n, values=None):
        buf = np.zeros(n) if values is None else _f64(values)
        self._check(self.lib.rn_debug_cut_buffer(self.h, 0 if values is None else 1, buf.ctypes.data, buf.size))
        return buf

    def setCutStage(self, stage, moments=None):
        """moments = partition.cut_children_moments(full_tree, stage), required when nranks > 1."""
        self._check(self.lib.rn_set_cut_stage(self.h, int(stage)))
        if moments is not None:
            E, P = _f64(moments[0]), _f64(moments[1])
            self._check(self.lib.rn_set_cut_children_moments(self.h, E.ctypes.data, P.ctypes.data, P.size))

    def shardInfo(self):
        out = np.zeros(7, dtype=np.int32)
        self._check(self.lib.rn_shard_info(self.h, out.ctypes.data))
        return dict(zip(("rank", "nranks", "cut_stage", "cut_parents", "comm_ranks", "local_nodes", "full_nodes"), (int(v) for v in out)))

    def shardGlobalNodes(self):
        n = self.shardInfo()["local_nodes"]
        out = np.zeros(n, dtype=np.int32)
        self._check(self.lib.rn_shard_global_nodes(self.h, out.ctypes.data, n))
        return out

    def debugSetAllreduce(self, fn):
        """fn(dev_ptr, count, is_f64, op, stream) -> 0; called in place of ncclAllReduce (test facility)."""
        self._ar_cb = ALLREDUCE_FN(lambda user, buf, count, f64, op, stream: int(fn(buf, count, f64, op, stream))) if fn is not None else C.cast(None, ALLREDUCE_FN)
        self._check(self.lib.rn_debug_set_allreduce(self.h, self._ar_cb, None))

    def joinLocalGroup(self, group, rank):
        self._check(self.lib.rn_debug_local_group_join(self.h, group, int(rank)))

    def kernelInfo(self):
        out = np.zeros(8, dtype=np.int32)
        self._check(self.lib.rn_get_kernel_info(self.h, out.ctypes.data))
        keys = ("dual_stage", "dual_blocks", "dual_trips", "dual_pipe", "stream_G", "stream_NL", "chain_stage", "vlv_slab")
        return dict(zip(keys, (int(v) for v in out)))

    def counters(self):
        """rn_apg_iterate batch bookkeeping: dict(optimistic, exact, replayed, hold)."""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.rn_get_counters(self.h, out.ctypes.data))
        return dict(zip(("optimistic", "exact", "replayed", "hold"), (int(v) for v in out)))

    def historyParts(self, first, n):
        out = np.zeros(4 * n)
        self._check(self.lib.rn_get_history_parts(self.h, int(first), int(n), out.ctypes.data))
        return out.reshape(n, 4)


def tree_structs(tree, nx, nu, nv, nd):
    """(RnDims, RnTree, arrays to keep alive) of a tree dict in the reference's JSON schema."""
    N, K, nodes = (int(_s(tree, k)) for k in ("N", "K", "nodes"))
    dims = RnDims(nx, nu, nv, nd, N, K, nodes, int(_s(tree, "nNonLeafNodes")))
    keep = [_i32(tree[k]) for k in ("stages", "nodesPerStage", "nodesPerStageCumul", "ancestor", "nChildren", "nChildrenCumul")]
    keep.append(_f64(tree["probNode"]))
    if len(keep[1]) < N + 1 or len(keep[2]) < N + 2:
        raise RapidNetError("nodesPerStage needs N+1 and nodesPerStageCumul N+2 entries (ScenarioTree.cu:66-75)")
    return dims, RnTree(*[a.ctypes.data for a in keep]), keep


def default_cut_stage(tree, nx=1, nu=1, nv=1, nd=1):
    dims, t, _keep = tree_structs(tree, nx, nu, nv, nd)
    c = load().rn_default_cut_stage(C.byref(dims), C.byref(t))
    if c < 0:
        raise RapidNetError("rn_default_cut_stage failed (%d)" % c)
    return c


def partition_tree(tree, rank, nranks, cut_stage=0):
    """rn_partition_create on a tree dict: returns a dict with the local tree (reference JSON schema, like
    rapidnet_amd.partition.local_tree), 'globalNode', 'cutStage', 'momE' [parents, nd], 'momP' [parents]."""
    lib = load()
    nd, nu = int(_s(tree, "dimDemand")), int(_s(tree, "dimPrice"))
    dims, t, _keep = tree_structs(tree, 1, nu, 1, nd)
    ed, ep = _f64(tree["errorDemandNode"]), _f64(tree["errorPriceNode"])
    part = RnPartition()
    rc = lib.rn_partition_create(C.byref(dims), C.byref(t), ed.ctypes.data, ep.ctypes.data, int(rank), int(nranks), int(cut_stage), C.byref(part))
    if rc != 0:
        raise RapidNetError("rn_partition_create failed (%d): %s" % (rc, lib.rn_last_error(None).decode()))
    try:
        n, N = part.dims.nodes, part.dims.N
        iarr = lambda ptr, cnt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int)), (cnt,)).copy() if cnt else np.zeros(0, np.int32)
        darr = lambda ptr, cnt: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), (cnt,)).copy() if cnt else np.zeros(0)
        local = {
            "N": [N], "K": [part.dims.K], "dimDemand": [nd], "dimPrice": [nu], "nodes": [n], "nChildrenTot": [n - 1],
            "nNonLeafNodes": [part.dims.nNonLeafNodes],
            "stages": iarr(part.tree.stages, n).tolist(), "nodesPerStage": iarr(part.tree.nodesPerStage, N + 1).tolist(),
            "nodesPerStageCumul": iarr(part.tree.nodesPerStageCumul, N + 2).tolist(), "ancestor": iarr(part.tree.ancestor, n).tolist(),
            "nChildren": iarr(part.tree.nChildren, part.dims.nNonLeafNodes).tolist(), "nChildrenCumul": iarr(part.tree.nChildrenCumul, n).tolist(),
            "probNode": darr(part.tree.probNode, n).tolist(),
            "errorDemandNode": darr(part.errorDemandNode, n * nd).tolist(), "errorPriceNode": darr(part.errorPriceNode, n * nu).tolist(),
        }
        cc = np.bincount(np.asarray(local["ancestor"])[1:] - 1, minlength=n)
        local["leaves"] = (np.flatnonzero(cc == 0) + 1).tolist()
        local["children"] = [i + 1 for i in range(1, n)]
        return {"tree": local, "globalNode": iarr(part.globalNode, n), "cutStage": part.cutStage,
                "momE": darr(part.momE, part.nCutParents * nd).reshape(part.nCutParents, nd), "momP": darr(part.momP, part.nCutParents)}
    finally:
        lib.rn_partition_destroy(C.byref(part))


def guard_report():
    """(contexts checked at rn_destroy in guard mode, red-zone bytes found overwritten) of this process."""
    out = (C.c_long * 2)()
    load().rn_guard_report(C.addressof(out))
    return int(out[0]), int(out[1])


def peer_inbox_connect_local(solvers):
    """contexts of ONE process, in rank order, each with an inbox (peerInboxCreate): wire them to each other (tests)"""
    arr = (C.c_void_p * len(solvers))(*[s.h for s in solvers])
    rc = load().rn_debug_peer_inbox_connect_local(arr, len(solvers))
    if rc != 0:
        raise RapidNetError("rn_debug_peer_inbox_connect_local failed (%d): %s" % (rc, "; ".join(load().rn_last_error(s.h).decode() for s in solvers)))


def local_group_create(nranks):
    g = C.c_void_p()
    rc = load().rn_debug_local_group_create(int(nranks), C.byref(g))
    if rc != 0:
        raise RapidNetError("rn_debug_local_group_create failed (%d)" % rc)
    return g


def local_group_destroy(group):
    load().rn_debug_local_group_destroy(group)


def comm_library():
    """Path of the RCCL image librapidnet_hip bound (an already-loaded image is reused)."""
    buf = C.create_string_buffer(4096)
    rc = load().rn_comm_library(buf, 4096)
    if rc != 0:
        raise RapidNetError("rn_comm_library failed (%d)" % rc)
    return buf.value.decode()


def comm_unique_id():
    buf = C.create_string_buffer(128)
    rc = load().rn_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc != 0:
        raise RapidNetError("rn_comm_unique_id failed (%d)" % rc)
    return bytes(buf.raw)
