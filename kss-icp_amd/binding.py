"""ctypes binding of include/kssicp.h (libkssicp.so).

Host pointers are numpy arrays; device pointers are integers (e.g. torch `tensor.data_ptr()`).
No CPU fallback: a missing library or GPU raises KssError.
"""
import collections
import ctypes as C
import operator
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
NSUMS = 20
K_NN_SWEEP, K_CORR_REDUCE, K_PRESHAPE, K_ROT_SEARCH, K_POSE_APPLY, K_GRID_NN, K_GRID_BUILD, K_GRID_CHAIN, K_GRID_CHAIN_PASS, K_RESIDENT, K_RESIDENT_PASS = range(11)
NN_AUTO, NN_BRUTE, NN_GRID = 0, 1, 2
P2L_NSUMS = 32           # KSS_P2L_NSUMS: the point-to-plane sums record
STATE_DEGENERATE = 6     # KSS_STATE_DEGENERATE: a point-to-plane pass met a singular system
ERR_DEGENERATE = -7      # KSS_ERR_DEGENERATE
METRIC_POINT, METRIC_PLANE = 0, 1   # KSS_METRIC_*: the step of kss_icp_trimmed
TRIM_NINFO = 4           # KSS_TRIM_NINFO: {m candidates, k rank, tau, kept} of a trimmed pass
LOSS_L2, LOSS_HUBER, LOSS_TUKEY, LOSS_CAUCHY = 0, 1, 2, 3   # KSS_LOSS_*: the weight of kss_icp_robust
ROBUST_NINFO = 4         # KSS_ROBUST_NINFO: {m candidates, c2, sum of weights, cnt kept} of a robust pass
SIM_NINFO = 6            # KSS_SIM_NINFO: {m, k, tau, kept, s_k, s_acc after the pass} of a similarity pass
O2O_NINFO = 5            # KSS_O2O_NINFO: {u survivors, k, tau, kept, m candidates} of a one-to-one pass
VMAP_NINFO = 10          # KSS_VMAP_NINFO: {mapped targets, voxels, dims x y z, leaf, origin x y z, inv widened} of a voxel map
VMAP_NSTAT = 10          # KSS_VMAP_NSTAT: {N, mean x y z, S00 S01 S02 S11 S12 S22} of a voxel
VMAP_NINSERT = 4         # KSS_VMAP_NINSERT: {points added, points not mapped, points outside the box, voxels created} of an insert
VMAP_NSHIFT = 4          # KSS_VMAP_NSHIFT: {voxels kept, voxels dropped, mapped points dropped, delta} of a shift
VGICP_NINFO = 4          # KSS_VGICP_NINFO: {kept in the last pass, ns, [30] of the last pass, voxels of the map}
RECIP_NINFO = 6          # KSS_RECIP_NINFO: {r mutual winners, k, tau, kept, m candidates, u winners} of a reciprocal pass
F32, F64 = 0, 1

# every symbol include/kssicp.h declares (checked by tests/test_abi.py against the header text)
SYMBOLS = [
    "kss_version", "kss_status_string", "kss_last_error", "kss_ctx_create", "kss_ctx_create_on_stream",
    "kss_ctx_destroy", "kss_ctx_synchronize", "kss_ctx_stream", "kss_ctx_set_nn_mode", "kss_profile_enable", "kss_profile_reset",
    "kss_profile_get", "kss_profile_event_overhead", "kss_grid_stats", "kss_preshape_stats", "kss_preshape_stats_dev", "kss_preshape_stats_pair_dev", "kss_pose_apply", "kss_pose_apply_dev",
    "kss_nn", "kss_nn_dev", "kss_cov", "kss_cov_dev", "kss_rigid_from_sums", "kss_rotation_search",
    "kss_rotation_search_dev", "kss_grid_angles", "kss_rotation_candidates", "kss_icp_default_params", "kss_icp",
    "kss_icp_dev", "kss_icp_batch", "kss_icp_batch_dev", "kss_transform_apply", "kss_transform_apply_dev",
    "kss_pcr_qm", "kss_register", "kss_register_batch", "kss_gather_results", "kss_rccl_allreduce_sum", "kss_transform_apply_f32", "kss_downsample_fps", "kss_downsample_aivs", "kss_downsample_aivs_pair", "kss_downsample_octree", "kss_knn", "kss_knn_dev", "kss_normals", "kss_normals_orient",
    "kss_p2l_sums", "kss_p2l_sums_dev", "kss_rigid_from_p2l_sums", "kss_icp_p2l", "kss_icp_p2l_dev",
    "kss_trim_rank", "kss_trim_threshold", "kss_trim_threshold_dev", "kss_icp_trimmed", "kss_icp_trimmed_dev",
    "kss_icp_p2l_batch", "kss_icp_p2l_batch_dev", "kss_icp_trimmed_batch", "kss_icp_trimmed_batch_dev",
    "kss_trim_threshold_batch", "kss_trim_threshold_batch_dev",
    "kss_robust_default_params", "kss_robust_weight", "kss_robust_scale2", "kss_robust_sums", "kss_robust_sums_dev",
    "kss_icp_robust", "kss_icp_robust_dev", "kss_icp_robust_batch", "kss_icp_robust_batch_dev",
    "kss_gicp_default_params", "kss_gicp_metric", "kss_gicp_sums", "kss_gicp_sums_dev", "kss_icp_gicp", "kss_icp_gicp_dev",
    "kss_icp_gicp_batch", "kss_icp_gicp_batch_dev",
    "kss_symm_default_params", "kss_rigid_from_symm_sums", "kss_symm_sums", "kss_symm_sums_dev", "kss_icp_symm", "kss_icp_symm_dev",
    "kss_icp_symm_batch", "kss_icp_symm_batch_dev",
    "kss_symm_robust_sums", "kss_symm_robust_sums_dev", "kss_icp_symm_robust", "kss_icp_symm_robust_dev",
    "kss_icp_symm_robust_batch", "kss_icp_symm_robust_batch_dev",
    "kss_sim_default_params", "kss_sim_from_sums", "kss_sim_sums", "kss_sim_sums_dev", "kss_icp_sim", "kss_icp_sim_dev",
    "kss_icp_sim_batch", "kss_icp_sim_batch_dev",
    "kss_o2o_filter", "kss_o2o_filter_dev", "kss_o2o_filter_batch", "kss_o2o_filter_batch_dev", "kss_o2o_default_params",
    "kss_icp_o2o", "kss_icp_o2o_dev", "kss_icp_o2o_batch", "kss_icp_o2o_batch_dev",
    "kss_recip_filter", "kss_recip_filter_dev", "kss_recip_default_params", "kss_icp_recip", "kss_icp_recip_dev",
    "kss_recip_filter_batch", "kss_recip_filter_batch_dev", "kss_icp_recip_pairs", "kss_icp_recip_pairs_dev",
    "kss_vmap_default_params", "kss_vmap_create", "kss_vmap_create_dev", "kss_vmap_destroy", "kss_vmap_info", "kss_vmap_read",
    "kss_vmap_create_box", "kss_vmap_insert", "kss_vmap_insert_dev", "kss_vmap_window", "kss_vmap_shift", "kss_vmap_recentre",
    "kss_vmap_coarsen", "kss_vmap_coarsen_into", "kss_vmap_set_neighbourhood", "kss_vmap_neighbourhood",
    "kss_vgicp_sums", "kss_vgicp_sums_dev", "kss_icp_vgicp", "kss_icp_vgicp_dev",
    "kss_icp_vgicp_from", "kss_icp_vgicp_from_dev", "kss_icp_vgicp_c2f", "kss_icp_vgicp_c2f_dev",
    "kss_icp_vgicp_batch", "kss_icp_vgicp_batch_dev",
]


class KssError(RuntimeError):
    def __init__(self, status, where, detail=""):
        self.status = status
        msg = "%s failed: status %d" % (where, status)
        if detail:
            msg += " (%s)" % detail
        super().__init__(msg)


# kss_allreduce_fn: in-place sum over ranks of n doubles in host memory (kss_icp_params.allreduce)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int)


class RcclLink(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rccl_comm", C.c_void_p)]


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("max_corr_dist", C.c_double),
                ("transformation_epsilon", C.c_double), ("euclidean_fitness_epsilon", C.c_double),
                ("abs_mse_epsilon", C.c_double), ("min_correspondences", C.c_int),
                ("fixed_iterations", C.c_int), ("nn_fma", C.c_int), ("compute_fitness", C.c_int),
                ("nn_sources_per_thread", C.c_int), ("nn_target_splits", C.c_int), ("nn_mode", C.c_int),
                ("trace_sums", C.POINTER(C.c_double)), ("trace_Tk", C.POINTER(C.c_float)),
                ("trace_cap", C.c_int), ("trace_n", C.POINTER(C.c_int)),
                ("fitness_idx", C.POINTER(C.c_int32)), ("fitness_d2", C.POINTER(C.c_float)),
                ("allreduce", ALLREDUCE_FN), ("allreduce_user", C.c_void_p)]


class TrimParams(C.Structure):
    _fields_ = [("overlap", C.c_double), ("metric", C.c_int), ("trace_trim", C.POINTER(C.c_double))]


class SimParams(C.Structure):
    _fields_ = [("overlap", C.c_double), ("scale_min", C.c_double), ("scale_max", C.c_double), ("trace_sim", C.POINTER(C.c_double))]


class O2oParams(C.Structure):
    _fields_ = [("overlap", C.c_double), ("metric", C.c_int), ("trace_o2o", C.POINTER(C.c_double))]


class RecipParams(C.Structure):
    _fields_ = [("overlap", C.c_double), ("metric", C.c_int), ("trace_recip", C.POINTER(C.c_double))]


class RobustParams(C.Structure):
    _fields_ = [("loss", C.c_int), ("metric", C.c_int), ("scale", C.c_double), ("tune", C.c_double), ("min_scale", C.c_double),
                ("trace_robust", C.POINTER(C.c_double))]


class GicpParams(C.Structure):
    _fields_ = [("epsilon", C.c_double), ("normals_k", C.c_int)]


class VmapParams(C.Structure):
    _fields_ = [("leaf", C.c_double), ("normals_k", C.c_int)]


class SymmParams(C.Structure):
    _fields_ = [("normals_k", C.c_int), ("align_normals", C.c_int)]


class IcpResult(C.Structure):
    _fields_ = [("T", C.c_float * 16), ("fitness", C.c_double), ("last_mse", C.c_double),
                ("iterations", C.c_int32), ("converged", C.c_int32), ("state", C.c_int32), ("pair_id", C.c_int32)]

    def matrix(self):
        return np.array(self.T, dtype=np.float32).reshape(4, 4)


class Pose(C.Structure):
    _fields_ = [("shift", C.c_double * 3), ("center", C.c_double * 3), ("scale", C.c_double), ("angle", C.c_double * 3)]


class RegisterResult(C.Structure):
    _fields_ = [("scale", C.c_double), ("angle", C.c_double * 3), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("c_src", C.c_double * 3), ("c_tgt", C.c_double * 3), ("T_icp", C.c_float * 16), ("E_d_init", C.c_double), ("final_fitness", C.c_double),
                ("used_angle_list", C.c_int32), ("angle_index", C.c_int32), ("n_angle_list", C.c_int32),
                ("icp_iterations", C.c_int32), ("icp_converged", C.c_int32), ("grid", C.c_int32)]


def lib_path():
    return os.path.join(_HERE, "lib", "libkssicp.so")


def build_library(force=False):
    """Compile libkssicp.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", _HERE, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", _HERE, "-j4"], stdout=subprocess.DEVNULL)
    return lib_path()


def _declare(L):
    """restype / argtypes of every entry point of a loaded libkssicp.so."""
    vp, i64, dbl = C.c_void_p, C.c_int64, C.c_double
    L.kss_version.restype = C.c_int
    L.kss_status_string.restype = C.c_char_p
    L.kss_status_string.argtypes = [C.c_int]
    L.kss_last_error.restype = C.c_char_p
    L.kss_last_error.argtypes = [vp]
    L.kss_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.kss_ctx_create_on_stream.argtypes = [C.c_int, vp, C.POINTER(vp)]
    L.kss_ctx_destroy.argtypes = [vp]
    L.kss_ctx_synchronize.argtypes = [vp]
    L.kss_ctx_stream.restype = vp
    L.kss_ctx_stream.argtypes = [vp]
    L.kss_ctx_set_nn_mode.argtypes = [vp, C.c_int]
    L.kss_profile_enable.argtypes = [vp, C.c_int]
    L.kss_profile_reset.argtypes = [vp]
    L.kss_grid_stats.argtypes = [vp, vp]
    L.kss_profile_get.argtypes = [vp, C.c_int, C.POINTER(dbl), C.POINTER(i64)]
    L.kss_profile_event_overhead.argtypes = [vp, C.POINTER(dbl)]
    L.kss_downsample_octree.argtypes = [vp, vp, i64, vp, i64, C.POINTER(i64), C.POINTER(dbl)]
    L.kss_normals_orient.argtypes = [vp, vp, i64, vp]
    L.kss_register_batch.argtypes = [vp, vp, vp, vp, vp, C.c_int, i64, dbl, C.c_int, C.c_int, vp, vp]
    for n in ("kss_preshape_stats", "kss_preshape_stats_dev"):
        getattr(L, n).argtypes = [vp, vp, C.c_int, i64, vp, C.POINTER(dbl)]
    L.kss_preshape_stats_pair_dev.argtypes = [vp, vp, i64, vp, i64, C.c_int, vp, C.POINTER(dbl), vp, C.POINTER(dbl)]
    for n in ("kss_pose_apply", "kss_pose_apply_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, C.POINTER(Pose), vp]
    for n in ("kss_nn", "kss_nn_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, vp]
    for n in ("kss_cov", "kss_cov_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, i64, i64, dbl, vp]
    L.kss_rigid_from_sums.argtypes = [vp, vp]
    for n in ("kss_p2l_sums", "kss_p2l_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, i64, i64, dbl, vp]
    L.kss_rigid_from_p2l_sums.argtypes = [vp, vp]
    for n in ("kss_icp_p2l", "kss_icp_p2l_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    L.kss_trim_rank.argtypes = [i64, dbl, C.POINTER(i64)]
    for n in ("kss_trim_threshold", "kss_trim_threshold_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, dbl, dbl, vp]
    for n in ("kss_icp_trimmed", "kss_icp_trimmed_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(TrimParams), C.POINTER(IcpResult), vp]
    L.kss_sim_default_params.argtypes = [C.POINTER(SimParams)]
    L.kss_sim_from_sums.argtypes = [vp, dbl, dbl, vp, C.POINTER(dbl)]
    for n in ("kss_sim_sums", "kss_sim_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, i64, i64, dbl, vp]
    for n in ("kss_icp_sim", "kss_icp_sim_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, C.POINTER(IcpParams), C.POINTER(SimParams), C.POINTER(IcpResult), vp]
    for n in ("kss_icp_sim_batch", "kss_icp_sim_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(SimParams), vp, vp, vp]
    L.kss_o2o_default_params.argtypes = [C.POINTER(O2oParams)]
    for n in ("kss_o2o_filter", "kss_o2o_filter_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, i64, i64, dbl, vp, vp, vp]
    for n in ("kss_o2o_filter_batch", "kss_o2o_filter_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, C.c_int, dbl, vp, vp, vp]
    for n in ("kss_icp_o2o", "kss_icp_o2o_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(O2oParams), C.POINTER(IcpResult), vp]
    for n in ("kss_icp_o2o_batch", "kss_icp_o2o_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(O2oParams), vp, vp, vp]
    L.kss_recip_default_params.argtypes = [C.POINTER(RecipParams)]
    for n in ("kss_recip_filter", "kss_recip_filter_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, vp, dbl, C.c_int, vp, vp, vp]
    for n in ("kss_icp_recip", "kss_icp_recip_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(RecipParams), C.POINTER(IcpResult), vp]
    for n in ("kss_recip_filter_batch", "kss_recip_filter_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, C.c_int, vp, vp, dbl, C.c_int, vp, vp, vp]
    for n in ("kss_icp_recip_pairs", "kss_icp_recip_pairs_dev"):      # (the many-pairs form; the C symbol is spelled _pairs: include/kssicp.h)
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(RecipParams), vp, vp, vp]
    L.kss_robust_default_params.argtypes = [C.c_int, C.c_int, C.POINTER(RobustParams)]
    L.kss_robust_weight.argtypes = [C.c_int, dbl, dbl, C.POINTER(dbl)]
    L.kss_robust_scale2.argtypes = [C.c_int, dbl, C.c_float, dbl, C.POINTER(dbl)]
    for n in ("kss_robust_sums", "kss_robust_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, i64, i64, dbl, C.POINTER(RobustParams), vp, vp]
    for n in ("kss_icp_robust", "kss_icp_robust_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(RobustParams), C.POINTER(IcpResult), vp]
    L.kss_gicp_default_params.argtypes = [C.POINTER(GicpParams)]
    L.kss_gicp_metric.argtypes = [vp, vp, dbl, vp, C.POINTER(C.c_int)]
    for n in ("kss_gicp_sums", "kss_gicp_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, dbl, vp, C.POINTER(GicpParams), vp]
    for n in ("kss_icp_gicp", "kss_icp_gicp_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(GicpParams), C.POINTER(IcpResult)]
    L.kss_vmap_default_params.argtypes = [C.POINTER(VmapParams)]
    for n in ("kss_vmap_create", "kss_vmap_create_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, C.POINTER(VmapParams), C.POINTER(vp)]
    L.kss_vmap_destroy.argtypes = [vp, vp]
    L.kss_vmap_info.argtypes = [vp, vp]
    L.kss_vmap_read.argtypes = [vp, vp, vp, vp, i64, C.POINTER(i64)]
    L.kss_vmap_create_box.argtypes = [vp, vp, vp, C.POINTER(VmapParams), C.POINTER(vp)]
    for n in ("kss_vmap_insert", "kss_vmap_insert_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, i64, vp, vp, C.c_int, vp]
    L.kss_vmap_window.argtypes = [vp, vp]
    L.kss_vmap_shift.argtypes = [vp, vp, vp, vp]
    L.kss_vmap_recentre.argtypes = [vp, vp, vp, i64, vp, vp]
    L.kss_vmap_coarsen.argtypes = [vp, vp, C.c_int, C.POINTER(vp)]
    L.kss_vmap_coarsen_into.argtypes = [vp, vp, C.c_int, vp]
    L.kss_vmap_set_neighbourhood.argtypes = [vp, vp, C.c_int]
    L.kss_vmap_neighbourhood.argtypes = [vp, C.POINTER(C.c_int)]
    for n in ("kss_icp_vgicp_from", "kss_icp_vgicp_from_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, vp, C.POINTER(IcpParams), C.POINTER(GicpParams), C.POINTER(IcpResult), vp]
    for n in ("kss_icp_vgicp_c2f", "kss_icp_vgicp_c2f_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, C.c_int, vp, C.POINTER(IcpParams), C.POINTER(GicpParams), vp, vp]
    for n in ("kss_vgicp_sums", "kss_vgicp_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, i64, vp, dbl, vp, C.POINTER(GicpParams), vp]
    for n in ("kss_icp_vgicp", "kss_icp_vgicp_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, C.POINTER(IcpParams), C.POINTER(GicpParams), C.POINTER(IcpResult), vp]
    for n in ("kss_icp_vgicp_batch", "kss_icp_vgicp_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, C.c_int, vp, C.POINTER(IcpParams), C.POINTER(GicpParams), vp, vp, vp]
    for n in ("kss_icp_p2l_batch", "kss_icp_p2l_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), vp]
    for n in ("kss_icp_trimmed_batch", "kss_icp_trimmed_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(TrimParams), vp, vp, vp]
    for n in ("kss_icp_robust_batch", "kss_icp_robust_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(RobustParams), vp, vp, vp]
    L.kss_symm_default_params.argtypes = [C.POINTER(SymmParams)]
    L.kss_rigid_from_symm_sums.argtypes = [vp, vp]
    for n in ("kss_symm_sums", "kss_symm_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, dbl, vp, C.POINTER(SymmParams), vp]
    for n in ("kss_icp_symm", "kss_icp_symm_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(SymmParams), C.POINTER(IcpResult)]
    for n in ("kss_symm_robust_sums", "kss_symm_robust_sums_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, i64, i64, dbl, vp, C.POINTER(SymmParams), C.POINTER(RobustParams), vp, vp]
    for n in ("kss_icp_symm_robust", "kss_icp_symm_robust_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, vp, i64, vp, C.POINTER(IcpParams), C.POINTER(SymmParams), C.POINTER(RobustParams),
                                  C.POINTER(IcpResult), vp]
    for n in ("kss_icp_gicp_batch", "kss_icp_gicp_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(GicpParams), vp, vp]
    for n in ("kss_icp_symm_batch", "kss_icp_symm_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(SymmParams), vp, vp]
    for n in ("kss_icp_symm_robust_batch", "kss_icp_symm_robust_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), C.POINTER(SymmParams), vp,
                                  C.POINTER(RobustParams), vp, vp, vp]
    for n in ("kss_trim_threshold_batch", "kss_trim_threshold_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, C.c_int, dbl, vp, vp]
    for n in ("kss_rotation_search", "kss_rotation_search_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, dbl, vp, i64, C.POINTER(C.c_int)]
    L.kss_grid_angles.argtypes = [dbl, vp, C.c_int]
    L.kss_rotation_candidates.argtypes = [vp, C.c_int, dbl, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.kss_icp_default_params.argtypes = [C.POINTER(IcpParams)]
    for n in ("kss_icp", "kss_icp_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, C.POINTER(IcpParams), C.POINTER(IcpResult)]
    for n in ("kss_icp_batch", "kss_icp_batch_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(IcpParams), vp]
    for n in ("kss_transform_apply", "kss_transform_apply_dev"):
        getattr(L, n).argtypes = [vp, vp, vp, i64, vp]
    L.kss_pcr_qm.argtypes = [vp, vp, i64, vp, i64, vp]
    L.kss_transform_apply_f32.argtypes = [vp, vp, vp, i64, vp]
    L.kss_downsample_fps.argtypes = [vp, vp, i64, i64, vp, vp]
    L.kss_downsample_aivs.argtypes = [vp, vp, i64, i64, vp, i64, C.POINTER(i64), vp]
    L.kss_downsample_aivs_pair.argtypes = [vp, vp, i64, i64, vp, i64, C.POINTER(i64), vp, vp, i64, i64, vp, i64, C.POINTER(i64), vp, C.POINTER(C.c_int)]
    for n in ("kss_knn", "kss_knn_dev"):
        getattr(L, n).argtypes = [vp, vp, i64, vp, i64, C.c_int, vp, vp]
    L.kss_normals.argtypes = [vp, vp, i64, C.c_int, vp]
    L.kss_register.argtypes = [vp, vp, i64, vp, i64, vp, i64, dbl, C.c_int, vp, C.POINTER(RegisterResult)]
    L.kss_gather_results.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp]
    return L


_LIB = None


def load_library(path=None):
    """The product library, loaded and declared once.  With a path: a second, uncached handle on that build of libkssicp.so
    (Context(lib=...) runs on it; tools that compare two builds in one process)."""
    global _LIB
    if path is None and _LIB is not None:
        return _LIB
    p = lib_path() if path is None else os.path.abspath(path)
    if not os.path.exists(p):
        raise KssError(-4, "load_library", "libkssicp.so not built: run __graft_entry__.build() (no CPU fallback exists)"
                       if path is None else "%s does not exist" % p)
    # One HIP runtime per process: PyTorch ships its own libamdhip64.so; if libkssicp.so pulled in /opt/rocm's copy
    # first, torch would later load a second runtime and see no devices.  Importing torch first (when it is installed)
    # makes both resolve to the same library.  KSS_NO_TORCH=1 skips this for hosts that never use torch.
    if "torch" not in sys.modules and not os.environ.get("KSS_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = _declare(C.CDLL(p))
    if path is None:
        _LIB = L
    return L


def exported_symbols():
    L = load_library()
    return [s for s in SYMBOLS if hasattr(L, s)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 3)


# ---- host-only helpers (no GPU needed) ---------------------------------------------------------------
def grid_angles(step):
    L = load_library()
    buf = np.empty(256, np.float64)
    g = L.kss_grid_angles(float(step), _p(buf), 256)
    if g < 0:
        raise KssError(g, "kss_grid_angles")
    return buf[:g].copy()


def rotation_candidates(err, step):
    L = load_library()
    err = np.ascontiguousarray(err, dtype=np.float64)
    g = err.shape[0]
    best = np.empty(3, np.float64)
    alist = np.empty(3 * g ** 3, np.float64)
    nl = C.c_int(0)
    rc = L.kss_rotation_candidates(_p(err), g, float(step), _p(best), _p(alist), g ** 3, C.byref(nl))
    if rc != 0:
        raise KssError(rc, "kss_rotation_candidates")
    return best, alist[:3 * nl.value].reshape(-1, 3).copy()


def rigid_from_sums(sums):
    L = load_library()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    T = np.empty(16, np.float32)
    rc = L.kss_rigid_from_sums(_p(s), _p(T))
    if rc != 0:
        raise KssError(rc, "kss_rigid_from_sums")
    return T.reshape(4, 4)


def trim_rank(m, overlap):
    """kss_trim_rank: the rank k of trimmed ICP for m candidates (host only)."""
    L = load_library()
    k = C.c_int64(0)
    rc = L.kss_trim_rank(int(m), float(overlap), C.byref(k))
    if rc != 0:
        raise KssError(rc, "kss_trim_rank")
    return k.value


def sim_params(**kw):
    """kss_sim_default_params (overlap 1, scale_min 0.5, scale_max 2), then the fields given by keyword."""
    L = load_library()
    sp = SimParams()
    rc = L.kss_sim_default_params(C.byref(sp))
    if rc != 0:
        raise KssError(rc, "kss_sim_default_params")
    for k, v in kw.items():
        if k in ("overlap", "scale_min", "scale_max"):
            setattr(sp, k, float(v))
        else:
            raise AttributeError(k)
    return sp


def o2o_params(**kw):
    """kss_o2o_default_params (overlap 1, point metric), then the fields given by keyword."""
    L = load_library()
    op = O2oParams()
    rc = L.kss_o2o_default_params(C.byref(op))
    if rc != 0:
        raise KssError(rc, "kss_o2o_default_params")
    for k, v in kw.items():
        if not hasattr(op, k):
            raise AttributeError(k)
        setattr(op, k, v)
    return op


def recip_params(**kw):
    """kss_recip_default_params (overlap 1, point metric), then the fields given by keyword."""
    L = load_library()
    rp = RecipParams()
    rc = L.kss_recip_default_params(C.byref(rp))
    if rc != 0:
        raise KssError(rc, "kss_recip_default_params")
    for k, v in kw.items():
        if not hasattr(rp, k):
            raise AttributeError(k)
        setattr(rp, k, v)
    return rp


def sim_from_sums(sums, lo=0.5, hi=2.0):
    """kss_sim_from_sums: (T, s_k, status) -- the similarity step from an NSUMS record with the scale clamped to [lo, hi]; status 0,
    or ERR_DEGENERATE with T the identity and s_k = 1."""
    L = load_library()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.size != NSUMS:
        raise ValueError("need %d sums" % NSUMS)
    T = np.empty(16, np.float32)
    sk = C.c_double(0.0)
    rc = L.kss_sim_from_sums(_p(s), float(lo), float(hi), _p(T), C.byref(sk))
    if rc not in (0, ERR_DEGENERATE):
        raise KssError(rc, "kss_sim_from_sums")
    return T.reshape(4, 4), sk.value, rc


def robust_params(loss=LOSS_HUBER, metric=METRIC_POINT, **kw):
    """kss_robust_default_params for the loss and metric, then the fields given by keyword (scale, tune, min_scale)."""
    L = load_library()
    rp = RobustParams()
    rc = L.kss_robust_default_params(int(loss), int(metric), C.byref(rp))
    if rc != 0:
        raise KssError(rc, "kss_robust_default_params")
    for k, v in kw.items():
        if k not in ("scale", "tune", "min_scale"):
            raise AttributeError(k)
        setattr(rp, k, float(v))
    return rp


def robust_weight(loss, x, c2):
    """kss_robust_weight: the weight of the squared residual x under the loss with squared scale c2 (host only)."""
    L = load_library()
    w = C.c_double(0.0)
    rc = L.kss_robust_weight(int(loss), float(x), float(c2), C.byref(w))
    if rc != 0:
        raise KssError(rc, "kss_robust_weight")
    return w.value


def robust_scale2(metric, tune, med_key, min_scale=0.0):
    """kss_robust_scale2: c2 of the automatic scale from the median key (a float32; host only)."""
    L = load_library()
    c2 = C.c_double(0.0)
    rc = L.kss_robust_scale2(int(metric), float(tune), C.c_float(float(np.float32(med_key))), float(min_scale), C.byref(c2))
    if rc != 0:
        raise KssError(rc, "kss_robust_scale2")
    return c2.value


def gicp_params(**kw):
    """kss_gicp_default_params (epsilon 1e-3, normals_k 20), then the fields given by keyword."""
    L = load_library()
    gp = GicpParams()
    rc = L.kss_gicp_default_params(C.byref(gp))
    if rc != 0:
        raise KssError(rc, "kss_gicp_default_params")
    for k, v in kw.items():
        if k == "epsilon":
            gp.epsilon = float(v)
        elif k == "normals_k":
            gp.normals_k = int(v)
        else:
            raise AttributeError(k)
    return gp


def vmap_params(**kw):
    """kss_vmap_default_params (leaf 0: the caller sets it, normals_k 20), then the fields given by keyword."""
    L = load_library()
    vp = VmapParams()
    rc = L.kss_vmap_default_params(C.byref(vp))
    if rc != 0:
        raise KssError(rc, "kss_vmap_default_params")
    for k, v in kw.items():
        if not hasattr(vp, k):
            raise AttributeError(k)
        setattr(vp, k, v)
    return vp


class VoxelMap:
    """A voxel map of one target cloud (kss_vmap): made by Context.vmap() / vmap_dev(), or empty over a box by Context.vmap_box(),
    it lives on the device until close() -- or until its context is closed, which frees it -- serves any number of
    Context.icp_vgicp() / vgicp_sums() calls and takes further clouds with insert()."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def info(self):
        """kss_vmap_info: the VMAP_NINFO doubles {mapped targets, voxels, dims x y z, leaf, origin x y z, inv widened}."""
        out = np.zeros(VMAP_NINFO, np.float64)
        rc = self.ctx.L.kss_vmap_info(self.h, _p(out))
        if rc != 0:
            raise KssError(rc, "kss_vmap_info")
        return out

    def read(self):
        """kss_vmap_read: (lin [nvox] int64 ascending, stats [nvox, VMAP_NSTAT] float64)."""
        n = C.c_int64(0)
        self.ctx._chk(self.ctx.L.kss_vmap_read(self.ctx.h, self.h, None, None, 0, C.byref(n)), "kss_vmap_read")
        lin = np.zeros(n.value, np.int64)
        stats = np.zeros((n.value, VMAP_NSTAT), np.float64)
        self.ctx._chk(self.ctx.L.kss_vmap_read(self.ctx.h, self.h, _p(lin), _p(stats), n.value, C.byref(n)), "kss_vmap_read")
        return lin, stats

    def _insert(self, name, pts, n, normals, T, normals_k):
        Tm = None if T is None else np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        info = np.zeros(VMAP_NINSERT, np.float64)
        self.ctx._chk(getattr(self.ctx.L, name)(self.ctx.h, self.h, pts, int(n), normals, _p(Tm), int(normals_k), _p(info)), name)
        return info

    def insert(self, pts, normals=None, T=None, normals_k=20):
        """kss_vmap_insert: the cloud (n x 3) into the map at the pose T (a 4 x 4, None: as it is); normals: n x 3, or None to
        compute them at normals_k from the cloud as passed in.  The box never changes: points outside it are counted and left
        out.  Returns the VMAP_NINSERT doubles {points added, points not mapped, points outside the box, voxels created}."""
        a = _f32(pts)
        nr = _normals(normals, len(a), "cloud")
        return self._insert("kss_vmap_insert", _p(a), len(a), _p(nr), T, normals_k)

    def insert_dev(self, d_pts, n, d_normals, T=None, normals_k=20):
        """kss_vmap_insert_dev on device pointers (the normals pointer may be 0 / None; T stays a host array)."""
        return self._insert("kss_vmap_insert_dev", _dp(d_pts), n, _dp(d_normals), T, normals_k)

    def window(self):
        """kss_vmap_window: the window base, three int64 cells (0 until a shift)."""
        base = np.zeros(3, np.int64)
        rc = self.ctx.L.kss_vmap_window(self.h, _p(base))
        if rc != 0:
            raise KssError(rc, "kss_vmap_window")
        return base

    def shift(self, k):
        """kss_vmap_shift: the window moved by k whole cells per axis (3 integers); voxels that leave it are gone.  Returns the
        VMAP_NSHIFT doubles {voxels kept, voxels dropped, mapped points dropped, delta}."""
        kk = np.ascontiguousarray([int(x) for x in np.asarray(k).reshape(3)], dtype=np.int64)
        info = np.zeros(VMAP_NSHIFT, np.float64)
        self.ctx._chk(self.ctx.L.kss_vmap_shift(self.ctx.h, self.h, _p(kk), _p(info)), "kss_vmap_shift")
        return info

    def recentre(self, centre, slack=0):
        """kss_vmap_recentre: the shift that brings the cell of centre (3 floats) to the middle of the window, made on the axes
        where it is more than `slack` cells.  Returns (k [3] int64, the VMAP_NSHIFT doubles)."""
        c = np.ascontiguousarray(centre, dtype=np.float32).reshape(3)
        k = np.zeros(3, np.int64)
        info = np.zeros(VMAP_NSHIFT, np.float64)
        self.ctx._chk(self.ctx.L.kss_vmap_recentre(self.ctx.h, self.h, _p(c), int(slack), _p(k), _p(info)), "kss_vmap_recentre")
        return k, info

    def coarsen(self, k):
        """kss_vmap_coarsen: a NEW VoxelMap whose voxels are k x k x k blocks of this one's (k in 2..8), summed from the kept
        f64 sums: leaf k times as large, the same lattice anchor.  It is a map of its own and outlives this one."""
        h = C.c_void_p()
        self.ctx._chk(self.ctx.L.kss_vmap_coarsen(self.ctx.h, self.h, int(k), C.byref(h)), "kss_vmap_coarsen")
        return VoxelMap(self.ctx, h)

    def coarsen_into(self, dst, k):
        """kss_vmap_coarsen_into: dst, a VoxelMap that coarsen(k) of this map made (or one of its lo, leaf, inv and dims), refilled
        from this map as it stands now -- whatever dst held before."""
        self.ctx._chk(self.ctx.L.kss_vmap_coarsen_into(self.ctx.h, self.h, int(k), dst.h if dst is not None else None),
                      "kss_vmap_coarsen_into")

    def set_neighbourhood(self, nb):
        """kss_vmap_set_neighbourhood: 1 (the source's own voxel, what every map starts at), 7 or 27 -- the voxels every later
        vgicp_sums / icp_vgicp* call on this map matches a source against, one correspondence per occupied one."""
        self.ctx._chk(self.ctx.L.kss_vmap_set_neighbourhood(self.ctx.h, self.h, int(nb)), "kss_vmap_set_neighbourhood")

    @property
    def neighbourhood(self):
        """kss_vmap_neighbourhood: the map's setting, 1, 7 or 27."""
        nb = C.c_int(0)
        rc = self.ctx.L.kss_vmap_neighbourhood(self.h, C.byref(nb))
        if rc != 0:
            raise KssError(rc, "kss_vmap_neighbourhood")
        return nb.value

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx._chk(self.ctx.L.kss_vmap_destroy(self.ctx.h, self.h), "kss_vmap_destroy")
        self.h = None


def gicp_metric(nq, m, epsilon=1e-3):
    """kss_gicp_metric: (M, ok) -- the six upper-triangle entries of the metric of one correspondence from the float32 target
    normal nq and the turned source normal m (float64), ok False when the correspondence is dropped (host only)."""
    L = load_library()
    a = np.ascontiguousarray(nq, dtype=np.float32).reshape(3)
    b = np.ascontiguousarray(m, dtype=np.float64).reshape(3)
    M = np.zeros(6, np.float64)
    ok = C.c_int(0)
    rc = L.kss_gicp_metric(_p(a), _p(b), float(epsilon), _p(M), C.byref(ok))
    if rc != 0:
        raise KssError(rc, "kss_gicp_metric")
    return M, bool(ok.value)


def rigid_from_p2l_sums(sums):
    """kss_rigid_from_p2l_sums: (T, status) -- status 0, or ERR_DEGENERATE with T the identity."""
    L = load_library()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.size != P2L_NSUMS:
        raise ValueError("need %d sums" % P2L_NSUMS)
    T = np.empty(16, np.float32)
    rc = L.kss_rigid_from_p2l_sums(_p(s), _p(T))
    if rc not in (0, ERR_DEGENERATE):
        raise KssError(rc, "kss_rigid_from_p2l_sums")
    return T.reshape(4, 4), rc


def symm_params(**kw):
    """kss_symm_default_params (normals_k 20, align_normals 1), then the fields given by keyword."""
    L = load_library()
    sp = SymmParams()
    rc = L.kss_symm_default_params(C.byref(sp))
    if rc != 0:
        raise KssError(rc, "kss_symm_default_params")
    for k, v in kw.items():
        if k in ("normals_k", "align_normals"):
            setattr(sp, k, int(v))
        else:
            raise AttributeError(k)
    return sp


def rigid_from_symm_sums(sums):
    """kss_rigid_from_symm_sums: (T, status) -- the symmetric step (two half rotations) from a P2L_NSUMS record; status 0, or
    ERR_DEGENERATE with T the identity."""
    L = load_library()
    s = np.ascontiguousarray(sums, dtype=np.float64)
    if s.size != P2L_NSUMS:
        raise ValueError("need %d sums" % P2L_NSUMS)
    T = np.empty(16, np.float32)
    rc = L.kss_rigid_from_symm_sums(_p(s), _p(T))
    if rc not in (0, ERR_DEGENERATE):
        raise KssError(rc, "kss_rigid_from_symm_sums")
    return T.reshape(4, 4), rc


# ---- the pair metrics: marshalling vocabulary and one record per metric ------------------
def _dp(a):
    """A device address (an integer, e.g. tensor.data_ptr()) as a C pointer; 0 / None is NULL."""
    return C.c_void_p(int(a)) if a else None


def _normals(normals, n, what=""):
    """normals as float32 triples of n rows, None staying None.  what: "source" / "target" where an entry takes both clouds'
    normals, "" where it takes the target's alone."""
    if normals is None:
        return None
    nr = _f32(normals)
    if len(nr) != n:
        raise ValueError(("%s normals must have one row per point" % what) if what else "normals must have one row per target point")
    return nr


def _per_pair(a, dtype, npairs, noun):
    """The per-pair array of a batch (overlaps, scales, epsilons as float64; aligns as int32), None staying None."""
    if a is None:
        return None
    v = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if len(v) != npairs:
        raise ValueError("%s must hold one entry per pair" % noun)
    return v


def _rot(Rn):
    return np.ascontiguousarray(Rn, dtype=np.float32).reshape(9) if Rn is not None else None


def _structs(m, given, *a):
    """The params structs of metric m: the caller's, and where one is None the record's default made from a (what the method's
    own signature offers for it: overlap and metric, loss and metric, loss, or nothing)."""
    make = m.make
    if len(make) == 1:                                   # (a metric has one struct or two; written out, this runs on every call)
        g, = given
        return (g if g is not None else make[0](*a),)
    g0, g1 = given
    return (g0 if g0 is not None else make[0](*a), g1 if g1 is not None else make[1](*a))


# The cloud arguments of a kss_icp_* entry in C order, by the record's `normals`, picked from (source, its count or offsets, its
# normals, target, its count or offsets, its normals); "map": the source with its normals, then a voxel map as the target;
# "scans": packed scans with their offsets and normals -- the one map they share follows the scan count (_icp_call).
_CLOUDS = {"both": operator.itemgetter(0, 1, 2, 3, 4, 5), "target": operator.itemgetter(0, 1, 3, 4, 5),
           "none": operator.itemgetter(0, 1, 3, 4), "map": operator.itemgetter(0, 1, 2, 3), "scans": operator.itemgetter(0, 1, 2)}


# What differs between the kss_icp_* families, and nothing else:
#   single, many   the C symbols of the single pair and of the many-pairs form (their _dev twins add the suffix)
#   sums           the C symbol of the one-pass record, None where there is none
#   normals        "none", "target" or "both": which normals follow the clouds ("map": the source's, then a voxel map as the target)
#   make           one default maker per extra params struct, in C order (_structs() calls them; the trimmed families' struct is
#                  no default: their methods always make it from their own overlap and metric)
#   trace          the per-pass trace field of the LAST struct, rows ninfo wide; None: no such trace
#   info, ninfo    the result key and width of the per-call info record (ninfo doubles, a batch: a row per pair); None: none
#   per_pair       (noun, dtype) of the per-pair array that follows each struct in the many-pairs form
#   ncol           the width of a trace_sums row; None: NSUMS or P2L_NSUMS by the last struct's metric
Metric = collections.namedtuple("Metric", "single many sums normals make trace info ninfo per_pair ncol")
_OVERLAPS, _SCALES, _EPSILONS, _ALIGNS = ("overlaps", np.float64), ("scales", np.float64), ("epsilons", np.float64), ("aligns", np.int32)
_ICP = Metric("kss_icp", "kss_icp_batch", None, "none", (), None, None, 0, (), NSUMS)
_P2L = Metric("kss_icp_p2l", "kss_icp_p2l_batch", "kss_p2l_sums", "target", (), None, None, 0, (), P2L_NSUMS)
_TRIMMED = Metric("kss_icp_trimmed", "kss_icp_trimmed_batch", None, "target", (TrimParams,), "trace_trim", "trim_info", TRIM_NINFO,
                  (_OVERLAPS,), None)
_O2O = Metric("kss_icp_o2o", "kss_icp_o2o_batch", None, "target", (O2oParams,), "trace_o2o", "o2o_info", O2O_NINFO, (_OVERLAPS,), None)
_RECIP = Metric("kss_icp_recip", "kss_icp_recip_pairs", None, "target", (RecipParams,), "trace_recip", "recip_info", RECIP_NINFO,
                (_OVERLAPS,), None)          # (the many-pairs form is spelled _pairs: include/kssicp.h)
_SIM = Metric("kss_icp_sim", "kss_icp_sim_batch", "kss_sim_sums", "none", (sim_params,), "trace_sim", "sim_info", SIM_NINFO, (_OVERLAPS,), NSUMS)
_ROBUST = Metric("kss_icp_robust", "kss_icp_robust_batch", "kss_robust_sums", "target", (robust_params,), "trace_robust", "robust_info",
                 ROBUST_NINFO, (_SCALES,), None)
_GICP = Metric("kss_icp_gicp", "kss_icp_gicp_batch", "kss_gicp_sums", "both", (gicp_params,), None, None, 0, (_EPSILONS,), P2L_NSUMS)
_SYMM = Metric("kss_icp_symm", "kss_icp_symm_batch", "kss_symm_sums", "both", (symm_params,), None, None, 0, (_ALIGNS,), P2L_NSUMS)
_SYMM_ROBUST = Metric("kss_icp_symm_robust", "kss_icp_symm_robust_batch", "kss_symm_robust_sums", "both",
                      (lambda loss: symm_params(), lambda loss: robust_params(loss, METRIC_PLANE)), "trace_robust", "robust_info",
                      ROBUST_NINFO, (_ALIGNS, _SCALES), P2L_NSUMS)
_VGICP = Metric("kss_icp_vgicp", None, "kss_vgicp_sums", "map", (gicp_params,), None, "info", VGICP_NINFO, (), P2L_NSUMS)
_VGICP_BATCH = Metric(None, "kss_icp_vgicp_batch", None, "scans", (gicp_params,), None, "info", VGICP_NINFO, (_EPSILONS,), P2L_NSUMS)


# ---- context --------------------------------------------------------------------------------------------
class Context:
    """One kss_ctx (one GPU, one stream)."""

    def __init__(self, device=0, stream=None, lib=None):
        self.L = lib if lib is not None else load_library()
        self.h = C.c_void_p()
        if stream is None:
            rc = self.L.kss_ctx_create(int(device), C.byref(self.h))
        else:
            rc = self.L.kss_ctx_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise KssError(rc, "kss_ctx_create", self.L.kss_status_string(rc).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.kss_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, where):
        if rc != 0:
            raise KssError(rc, where, self.L.kss_last_error(self.h).decode() or self.L.kss_status_string(rc).decode())

    def set_nn_mode(self, mode):
        self._chk(self.L.kss_ctx_set_nn_mode(self.h, int(mode)), "kss_ctx_set_nn_mode")

    def synchronize(self):
        self._chk(self.L.kss_ctx_synchronize(self.h), "kss_ctx_synchronize")

    # ---- profiling
    def profile_enable(self, on=True):
        """False/0 = off, True/1 = time every launch, n > 1 = time every n-th launch of each kernel class."""
        self._chk(self.L.kss_profile_enable(self.h, int(on)), "kss_profile_enable")

    def profile_reset(self):
        self._chk(self.L.kss_profile_reset(self.h), "kss_profile_reset")

    def profile_event_overhead(self):
        ms = C.c_double(0)
        self._chk(self.L.kss_profile_event_overhead(self.h, C.byref(ms)), "kss_profile_event_overhead")
        return ms.value

    def profile_get(self, k):
        ms, n = C.c_double(0), C.c_int64(0)
        self._chk(self.L.kss_profile_get(self.h, k, C.byref(ms), C.byref(n)), "kss_profile_get")
        return ms.value, n.value

    def grid_stats(self):
        out = np.zeros(8, np.float64)
        self._chk(self.L.kss_grid_stats(self.h, _p(out)), "kss_grid_stats")
        return dict(zip(["h", "gx", "gy", "gz", "occupied_cells", "evaluations_per_pass", "n_src", "n_tgt"], out.tolist()))

    # ---- (a2)
    def preshape_stats(self, xyz):
        a = np.ascontiguousarray(xyz)
        if a.dtype == np.float32:
            a, dt = _f32(a), F32
        else:
            a, dt = _f64(a), F64
        c = np.empty(3, np.float64)
        r = C.c_double(0)
        self._chk(self.L.kss_preshape_stats(self.h, _p(a), dt, len(a), _p(c), C.byref(r)), "kss_preshape_stats")
        return c, r.value

    def preshape_stats_dev(self, dptr, dtype, n):
        c = np.empty(3, np.float64)
        r = C.c_double(0)
        self._chk(self.L.kss_preshape_stats_dev(self.h, C.c_void_p(int(dptr)), dtype, int(n), _p(c), C.byref(r)), "kss_preshape_stats_dev")
        return c, r.value

    def preshape_stats_pair_dev(self, d_src, ns, d_tgt, nt, dtype):
        cs, ct = np.empty(3, np.float64), np.empty(3, np.float64)
        rs, rt = C.c_double(0), C.c_double(0)
        self._chk(self.L.kss_preshape_stats_pair_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt), dtype,
                                                     _p(cs), C.byref(rs), _p(ct), C.byref(rt)), "kss_preshape_stats_pair_dev")
        return (cs, rs.value), (ct, rt.value)

    # ---- (a7)
    @staticmethod
    def make_pose(shift, center, scale, angle):
        p = Pose()
        for k in range(3):
            p.shift[k] = float(shift[k]); p.center[k] = float(center[k]); p.angle[k] = float(angle[k])
        p.scale = float(scale)
        return p

    def pose_apply(self, pts, pose):
        a = _f64(pts)
        out = np.empty_like(a)
        self._chk(self.L.kss_pose_apply(self.h, _p(a), len(a), C.byref(pose), _p(out)), "kss_pose_apply")
        return out

    def pose_apply_dev(self, d_in, n, pose, d_out):
        self._chk(self.L.kss_pose_apply_dev(self.h, C.c_void_p(int(d_in)), int(n), C.byref(pose), C.c_void_p(int(d_out))), "kss_pose_apply_dev")

    def transform_apply(self, T, pts):
        a = _f64(pts)
        Tm = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        out = np.empty_like(a)
        self._chk(self.L.kss_transform_apply(self.h, _p(Tm), _p(a), len(a), _p(out)), "kss_transform_apply")
        return out

    # ---- (a8)
    def nn(self, src, tgt):
        s, t = _f32(src), _f32(tgt)
        idx = np.empty(len(s), np.int32)
        d2 = np.empty(len(s), np.float32)
        self._chk(self.L.kss_nn(self.h, _p(s), len(s), _p(t), len(t), _p(idx), _p(d2)), "kss_nn")
        return idx, d2

    def nn_dev(self, d_src, ns, d_tgt, nt, d_idx, d_d2):
        self._chk(self.L.kss_nn_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                    C.c_void_p(int(d_idx)) if d_idx else None, C.c_void_p(int(d_d2)) if d_d2 else None), "kss_nn_dev")

    # ---- (a10)
    def cov(self, src, tgt, idx, max_d2=1.0):
        s, t = _f32(src), _f32(tgt)
        i = np.ascontiguousarray(idx, dtype=np.int32)
        sums = np.empty(NSUMS, np.float64)
        self._chk(self.L.kss_cov(self.h, _p(s), _p(t), _p(i), len(s), len(t), float(max_d2), _p(sums)), "kss_cov")
        return sums

    # ---- (a4)
    def rotation_search(self, src_preshaped, tgt, step):
        s, t = _f64(src_preshaped), _f64(tgt)
        err = np.empty(40 ** 3, np.float64)
        g = C.c_int(0)
        self._chk(self.L.kss_rotation_search(self.h, _p(s), len(s), _p(t), len(t), float(step), _p(err), err.size, C.byref(g)), "kss_rotation_search")
        g = g.value
        return err[:g ** 3].reshape(g, g, g).copy()

    # ---- (a9)
    def icp_params(self, **kw):
        p = IcpParams()
        self.L.kss_icp_default_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        return p

    # ---- the pair metrics: one traced call under the host forms (single pair / batch) and the three _dev batch forms that trace;
    # one plain call for the records.  The untraced _dev ICP forms attach nothing and keep their literal calls: they are the thin
    # wrappers a caller times, and tests/test_binding_calls.py checks each of them against its symbol's argtypes.
    def _icp_call(self, m, dev, src, ns, sn, tgt, nt, tn, p, structs=(), arrays=None, so=None, trace_cap=0, fitness_corr=False):
        """The kss_icp_* entry of metric m -- the _dev twin if dev, the many-pairs form if the source offsets so are given -- on the
        marshalled clouds (src, its count ns, its normals sn; tgt, nt, tn the same of the target; a batch: the marshalled offsets
        for the counts), the IcpParams p, m's params structs and (a batch) the caller's per-pair array beside each, checked and
        converted here.  Every entry that can trace is called from here and nowhere else.  The trace and fitness_corr
        arrays, the latter sized for the sources of the pair (a batch: of pair 0), are attached to p and to m's last struct and
        detached again whether the call returns or raises.  Returns (the IcpResult, or the ctypes array of a batch; the info
        record or None; the dictionary of the extras)."""
        single, many, _, normals, _, trace, key, ninfo, per_pair, ncol = m
        batch = so is not None
        args = [self.h, *_CLOUDS[normals]((src, ns, sn, tgt, nt, tn))]
        if batch:
            npairs = len(so) - 1
            res = (IcpResult * npairs)()
            args.append(npairs)
            if normals == "scans":                         # (many scans against one map: the map follows their count)
                args.append(tgt)
            args.append(C.byref(p))
            for st, a, (noun, dtype) in zip(structs, arrays, per_pair):
                args.append(C.byref(st))
                args.append(_p(_per_pair(a, dtype, npairs, noun)))
            args.append(C.cast(res, C.c_void_p))
        else:
            res = IcpResult()
            args.append(C.byref(p))
            for st in structs:
                args.append(C.byref(st))
            args.append(C.byref(res))
        info = None
        if key:
            info = np.zeros((npairs, ninfo) if batch else ninfo, np.float64)
            args.append(_p(info))
        where = many if batch else single
        if dev:
            where += "_dev"
        if trace_cap <= 0 and not fitness_corr:            # nothing to attach: the plain checked call
            self._chk(getattr(self.L, where)(*args), where)
            return res, info, {}
        tp = structs[-1] if trace else None
        tr = fc = None
        try:
            if fitness_corr:
                if batch:
                    ns = int(so[1] - so[0]) if npairs > 0 else 0
                fc = (np.full(ns, -1, np.int32), np.full(ns, np.nan, np.float32))
                p.fitness_idx = fc[0].ctypes.data_as(C.POINTER(C.c_int32))
                p.fitness_d2 = fc[1].ctypes.data_as(C.POINTER(C.c_float))
            if trace_cap > 0:
                ncol = ncol or (P2L_NSUMS if tp.metric == METRIC_PLANE else NSUMS)
                tr = (np.zeros((trace_cap, ncol), np.float64), np.zeros((trace_cap, 16), np.float32), C.c_int(0),
                      np.zeros((trace_cap, ninfo), np.float64) if tp is not None else None)
                p.trace_sums = tr[0].ctypes.data_as(C.POINTER(C.c_double))
                p.trace_Tk = tr[1].ctypes.data_as(C.POINTER(C.c_float))
                p.trace_cap = trace_cap
                p.trace_n = C.pointer(tr[2])
                if tp is not None:
                    setattr(tp, trace, tr[3].ctypes.data_as(C.POINTER(C.c_double)))
            self._chk(getattr(self.L, where)(*args), where)
        finally:
            if tr:
                p.trace_sums = None; p.trace_Tk = None; p.trace_cap = 0; p.trace_n = None
                if tp is not None:
                    setattr(tp, trace, None)
            if fc:
                p.fitness_idx = None; p.fitness_d2 = None
        extra = {}
        if tr:
            n = tr[2].value
            extra["trace_sums"] = tr[0][:n].copy()
            extra["trace_Tk"] = tr[1][:n].reshape(-1, 4, 4).copy()
            if tp is not None:
                extra[trace] = tr[3][:n].copy()
        if fc:
            extra["fitness_idx"], extra["fitness_d2"] = fc
        return res, info, extra

    @staticmethod
    def _result(m, res, info, extra):
        """The result dictionary of icp(), with the extras and m's info record under m's key."""
        out = {"T": res.matrix(), "iterations": res.iterations, "converged": bool(res.converged),
               "state": res.state, "fitness": res.fitness, "last_mse": res.last_mse}
        out.update(extra)
        if m.info:
            out[m.info] = info
        return out

    @staticmethod
    def _offsets(src_off, tgt_off):
        so = np.ascontiguousarray(src_off, dtype=np.int64)
        to = np.ascontiguousarray(tgt_off, dtype=np.int64)
        if len(so) != len(to) or len(so) < 1:
            raise ValueError("src_off and tgt_off must hold npairs + 1 entries each")
        return so, to

    def _pair(self, m, src, tgt, src_normals, tgt_normals, params, structs, trace_cap, fitness_corr):
        """Host arrays, one pair: the result dictionary."""
        s, t = _f32(src), _f32(tgt)
        sn = _normals(src_normals, len(s), "source")
        tn = _normals(tgt_normals, len(t), "target" if m.normals == "both" else "")
        p = params if params is not None else self.icp_params()
        res, info, extra = self._icp_call(m, False, _p(s), len(s), _p(sn), _p(t), len(t), _p(tn), p, structs, None, None, trace_cap,
                                          fitness_corr)
        return self._result(m, res, info, extra)

    def _pairs(self, m, src_all, src_off, tgt_all, tgt_off, src_normals_all, tgt_normals_all, params, structs, per_pair, trace_cap,
               fitness_corr):
        """Host arrays, many pairs: (list of IcpResult, [info of every pair,] extras of pair 0)."""
        s, t = _f32(src_all), _f32(tgt_all)
        sn = _normals(src_normals_all, len(s), "source")
        tn = _normals(tgt_normals_all, len(t), "target" if m.normals == "both" else "")
        so, to = self._offsets(src_off, tgt_off)
        p = params if params is not None else self.icp_params()
        res, info, extra = self._icp_call(m, False, _p(s), _p(so), _p(sn), _p(t), _p(to), _p(tn), p, structs, per_pair, so, trace_cap,
                                          fitness_corr)
        return (list(res), info, extra) if m.info else (list(res), extra)

    def _pairs_dev_traced(self, m, d_src_all, src_off, d_tgt_all, tgt_off, d_src_normals_all, d_tgt_normals_all, params, structs, per_pair,
                          trace_cap):
        """Device pointers, many pairs, of the families on both clouds' normals (gicp, symm, symm_robust): the only _dev forms that
        trace.  They take a trace_cap, accept params None and return pair 0's extras behind the list (and the info)."""
        so, to = self._offsets(src_off, tgt_off)
        p = params if params is not None else self.icp_params()
        res, info, extra = self._icp_call(m, True, _dp(d_src_all), _p(so), _dp(d_src_normals_all), _dp(d_tgt_all), _p(to),
                                          _dp(d_tgt_normals_all), p, structs, per_pair, so, trace_cap)
        return (list(res), info, extra) if m.info else (list(res), extra)

    def _sums(self, m, dev, args, structs=(), ncol=P2L_NSUMS, with_info=False):
        """The one-pass record of metric m (kss_*_sums, its _dev twin if dev), a plain checked call: args, m's structs, the sums
        and, for the robust records, the info.  Returns sums, or (sums, info)."""
        where = m.sums + ("_dev" if dev else "")
        sums = np.zeros(ncol, np.float64)
        info = np.zeros(m.ninfo, np.float64) if with_info else None
        self._chk(getattr(self.L, where)(self.h, *args, *[C.byref(st) for st in structs], _p(sums), *([_p(info)] if with_info else [])),
                  where)
        return (sums, info) if with_info else sums

    def _sums_both(self, m, src, src_normals, tgt, tgt_normals, idx, max_d2, Rn, structs, with_info=False):
        """_sums of a metric on both clouds' normals, host arrays."""
        s, t = _f32(src), _f32(tgt)
        sn, tn = _normals(src_normals, len(s), "source"), _normals(tgt_normals, len(t), "target")
        i = np.ascontiguousarray(idx, dtype=np.int32)
        return self._sums(m, False, (_p(s), _p(sn), _p(t), _p(tn), _p(i), len(s), len(t), float(max_d2), _p(_rot(Rn))), structs,
                          with_info=with_info)

    def _sums_both_dev(self, m, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2, Rn, structs, with_info=False):
        """_sums of a metric on both clouds' normals, device pointers (Rn stays a host array)."""
        return self._sums(m, True, (_dp(d_src), _dp(d_src_normals), _dp(d_tgt), _dp(d_tgt_normals), _dp(d_idx), int(n), int(nt),
                                    float(max_d2), _p(_rot(Rn))), structs, with_info=with_info)

    def icp(self, src, tgt, params=None, trace_cap=0, fitness_corr=False):
        return self._pair(_ICP, src, tgt, None, None, params, (), trace_cap, fitness_corr)

    # ---- point-to-plane
    def p2l_sums(self, src, tgt, normals, idx, max_d2=1.0):
        s, t, nr = _f32(src), _f32(tgt), _f32(normals)
        i = np.ascontiguousarray(idx, dtype=np.int32)
        return self._sums(_P2L, False, (_p(s), _p(t), _p(nr), _p(i), len(s), len(t), float(max_d2)))

    def p2l_sums_dev(self, d_src, d_tgt, d_normals, d_idx, n, nt, max_d2=1.0):
        return self._sums(_P2L, True, (_dp(d_src), _dp(d_tgt), _dp(d_normals), _dp(d_idx), int(n), int(nt), float(max_d2)))

    def icp_p2l(self, src, tgt, normals=None, params=None, trace_cap=0, fitness_corr=False):
        """Point-to-plane ICP (kss_icp_p2l).  normals: nt x 3 target normals, or None to have the library compute them
        (kss_normals' definition, k = 20, rounded to float).  Same result dictionary as icp(); trace_sums rows hold P2L_NSUMS."""
        return self._pair(_P2L, src, tgt, None, normals, params, (), trace_cap, fitness_corr)

    def icp_p2l_dev(self, d_src, ns, d_tgt, nt, d_normals, params):
        """kss_icp_p2l_dev on device pointers (d_normals may be 0 / None); returns the IcpResult."""
        res = IcpResult()
        self._chk(self.L.kss_icp_p2l_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                         C.c_void_p(int(d_normals)) if d_normals else None, C.byref(params), C.byref(res)),
                  "kss_icp_p2l_dev")
        return res

    # ---- trimmed ICP
    def trim_threshold(self, d2, max_d2=1.0, overlap=0.5):
        """kss_trim_threshold: {m, k, tau, kept} of the squared distances d2 (float32) as a float64 array of TRIM_NINFO."""
        d = np.ascontiguousarray(d2, dtype=np.float32).reshape(-1)
        info = np.zeros(TRIM_NINFO, np.float64)
        self._chk(self.L.kss_trim_threshold(self.h, _p(d), len(d), float(max_d2), float(overlap), _p(info)), "kss_trim_threshold")
        return info

    def trim_threshold_dev(self, d_d2, n, max_d2=1.0, overlap=0.5):
        info = np.zeros(TRIM_NINFO, np.float64)
        self._chk(self.L.kss_trim_threshold_dev(self.h, _dp(d_d2), int(n), float(max_d2), float(overlap), _p(info)), "kss_trim_threshold_dev")
        return info

    def icp_trimmed(self, src, tgt, normals=None, overlap=0.5, metric=METRIC_POINT, params=None, trace_cap=0, fitness_corr=False):
        """Trimmed ICP (kss_icp_trimmed): per pass the closest `overlap` share of the correspondences within max_corr_dist is
        kept.  metric METRIC_POINT (normals must be None) or METRIC_PLANE (normals nt x 3, or None to have them computed).
        The result dictionary of icp_p2l() plus trace_trim (one {m, k, tau, kept} row per traced pass) and trim_info (the last
        pass's); trace_sums rows hold NSUMS or P2L_NSUMS doubles by metric."""
        return self._pair(_TRIMMED, src, tgt, None, normals, params, (TrimParams(float(overlap), int(metric), None),), trace_cap, fitness_corr)

    def icp_trimmed_dev(self, d_src, ns, d_tgt, nt, d_normals, params, overlap=0.5, metric=METRIC_POINT):
        """kss_icp_trimmed_dev on device pointers (d_normals may be 0 / None); returns (IcpResult, trim_info)."""
        res = IcpResult()
        tp = TrimParams(float(overlap), int(metric), None)
        info = np.zeros(TRIM_NINFO, np.float64)
        self._chk(self.L.kss_icp_trimmed_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                             C.c_void_p(int(d_normals)) if d_normals else None, C.byref(params), C.byref(tp),
                                             C.byref(res), _p(info)), "kss_icp_trimmed_dev")
        return res, info

    # ---- one-to-one ICP
    def o2o_filter(self, idx, d2, nt, max_d2=1.0, want_idx=True, want_d2=True, alias=False):
        """kss_o2o_filter: (idx_f, d2_f, m, u) of the NN map idx (int32) / d2 (float32) against nt targets; an output that is not
        wanted is None.  alias: the library writes into (copies of) the inputs themselves."""
        i = np.array(idx, dtype=np.int32).reshape(-1)
        d = np.array(d2, dtype=np.float32).reshape(-1)
        if len(i) != len(d):
            raise ValueError("idx and d2 must have one entry per source")
        io = (i if alias else np.empty_like(i)) if want_idx else None
        do = (d if alias else np.empty_like(d)) if want_d2 else None
        info = np.zeros(2, np.float64)
        self._chk(self.L.kss_o2o_filter(self.h, _p(i), _p(d), len(i), int(nt), float(max_d2), _p(io), _p(do), _p(info)), "kss_o2o_filter")
        return io, do, int(info[0]), int(info[1])

    def o2o_filter_dev(self, d_idx, d_d2, n, nt, max_d2=1.0, d_idx_out=None, d_d2_out=None):
        """kss_o2o_filter_dev on device pointers (an output may be 0 / None, or its input); returns (m, u)."""
        info = np.zeros(2, np.float64)
        self._chk(self.L.kss_o2o_filter_dev(self.h, _dp(d_idx), _dp(d_d2), int(n), int(nt), float(max_d2), _dp(d_idx_out), _dp(d_d2_out),
                                            _p(info)), "kss_o2o_filter_dev")
        return int(info[0]), int(info[1])

    def o2o_filter_batch(self, idx_all, d2_all, off, nts, max_d2=1.0):
        """kss_o2o_filter_batch: the filter of every segment [off[i], off[i + 1]) against nts[i] targets in one call.  Returns
        (idx_f, d2_f, info nseg x 2 = {m, u}); entries outside the segments are left as given."""
        i = np.array(idx_all, dtype=np.int32).reshape(-1)
        d = np.array(d2_all, dtype=np.float32).reshape(-1)
        o = np.ascontiguousarray(off, dtype=np.int64)
        nt = np.ascontiguousarray(nts, dtype=np.int64)
        if len(nt) != len(o) - 1:
            raise ValueError("nts must hold one entry per segment")
        io, do = i.copy(), d.copy()
        info = np.zeros((len(nt), 2), np.float64)
        self._chk(self.L.kss_o2o_filter_batch(self.h, _p(i), _p(d), _p(o), _p(nt), len(nt), float(max_d2), _p(io), _p(do), _p(info)),
                  "kss_o2o_filter_batch")
        return io, do, info

    def icp_o2o(self, src, tgt, normals=None, overlap=1.0, metric=METRIC_POINT, params=None, trace_cap=0, fitness_corr=False):
        """One-to-one ICP (kss_icp_o2o): of all sources that chose one target only the closest keeps its correspondence, then
        icp_trimmed()'s pass at `overlap` over the survivors.  Arguments and result dictionary as icp_trimmed(), with trace_o2o
        (one {u, k, tau, kept, m} row per traced pass) and o2o_info (the last pass's) in place of the trimmed records."""
        return self._pair(_O2O, src, tgt, None, normals, params, (O2oParams(float(overlap), int(metric), None),), trace_cap, fitness_corr)

    def icp_o2o_dev(self, d_src, ns, d_tgt, nt, d_normals, params, overlap=1.0, metric=METRIC_POINT):
        """kss_icp_o2o_dev on device pointers (d_normals may be 0 / None); returns (IcpResult, o2o_info)."""
        res = IcpResult()
        op = O2oParams(float(overlap), int(metric), None)
        info = np.zeros(O2O_NINFO, np.float64)
        self._chk(self.L.kss_icp_o2o_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                         C.c_void_p(int(d_normals)) if d_normals else None, C.byref(params), C.byref(op),
                                         C.byref(res), _p(info)), "kss_icp_o2o_dev")
        return res, info

    # ---- reciprocal ICP
    def recip_filter(self, src, tgt, idx, d2, max_d2=1.0, nn_fma=0, want_idx=True, want_d2=True, alias=False):
        """kss_recip_filter: (idx_f, d2_f, m, u, r) of the map idx (int32) / d2 (float32) from the sources src to the targets tgt
        (float32 triples); an output that is not wanted is None.  alias: the library writes into (copies of) the inputs themselves."""
        s, t = _f32(src), _f32(tgt)
        i = np.array(idx, dtype=np.int32).reshape(-1)
        d = np.array(d2, dtype=np.float32).reshape(-1)
        if len(i) != len(d) or len(i) != len(s):
            raise ValueError("idx and d2 must have one entry per source")
        io = (i if alias else np.empty_like(i)) if want_idx else None
        do = (d if alias else np.empty_like(d)) if want_d2 else None
        info = np.zeros(3, np.float64)
        self._chk(self.L.kss_recip_filter(self.h, _p(s), len(s), _p(t), len(t), _p(i), _p(d), float(max_d2), int(nn_fma), _p(io), _p(do),
                                          _p(info)), "kss_recip_filter")
        return io, do, int(info[0]), int(info[1]), int(info[2])

    def recip_filter_dev(self, d_src, n, d_tgt, nt, d_idx, d_d2, max_d2=1.0, nn_fma=0, d_idx_out=None, d_d2_out=None):
        """kss_recip_filter_dev on device pointers (an output may be 0 / None, or its input); returns (m, u, r)."""
        info = np.zeros(3, np.float64)
        self._chk(self.L.kss_recip_filter_dev(self.h, _dp(d_src), int(n), _dp(d_tgt), int(nt), _dp(d_idx), _dp(d_d2), float(max_d2),
                                              int(nn_fma), _dp(d_idx_out), _dp(d_d2_out), _p(info)), "kss_recip_filter_dev")
        return int(info[0]), int(info[1]), int(info[2])

    def icp_recip(self, src, tgt, normals=None, overlap=1.0, metric=METRIC_POINT, params=None, trace_cap=0, fitness_corr=False):
        """Reciprocal ICP (kss_icp_recip): a correspondence is kept only where source and target are each other's nearest, then
        icp_trimmed()'s pass at `overlap` over the mutual winners.  Arguments and result dictionary as icp_o2o(), with trace_recip
        (one {r, k, tau, kept, m, u} row per traced pass) and recip_info (the last pass's)."""
        return self._pair(_RECIP, src, tgt, None, normals, params, (RecipParams(float(overlap), int(metric), None),), trace_cap, fitness_corr)

    def icp_recip_dev(self, d_src, ns, d_tgt, nt, d_normals, params, overlap=1.0, metric=METRIC_POINT):
        """kss_icp_recip_dev on device pointers (d_normals may be 0 / None); returns (IcpResult, recip_info)."""
        res = IcpResult()
        rp = RecipParams(float(overlap), int(metric), None)
        info = np.zeros(RECIP_NINFO, np.float64)
        self._chk(self.L.kss_icp_recip_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                           C.c_void_p(int(d_normals)) if d_normals else None, C.byref(params), C.byref(rp),
                                           C.byref(res), _p(info)), "kss_icp_recip_dev")
        return res, info

    # ---- similarity ICP
    def sim_sums(self, src, tgt, idx, max_d2=1.0):
        """kss_sim_sums: the untrimmed NSUMS record of the similarity step for given correspondences ([17] = the kept sources' sum
        of squares)."""
        s, t = _f32(src), _f32(tgt)
        i = np.ascontiguousarray(idx, dtype=np.int32)
        return self._sums(_SIM, False, (_p(s), _p(t), _p(i), len(s), len(t), float(max_d2)), ncol=NSUMS)

    def sim_sums_dev(self, d_src, d_tgt, d_idx, n, nt, max_d2=1.0):
        return self._sums(_SIM, True, (_dp(d_src), _dp(d_tgt), _dp(d_idx), int(n), int(nt), float(max_d2)), ncol=NSUMS)

    def icp_sim(self, src, tgt, sp=None, params=None, trace_cap=0, fitness_corr=False):
        """Similarity ICP (kss_icp_sim): trimmed ICP on the point metric with Umeyama's scale in the solve, the accumulated scale
        kept in [sp.scale_min, sp.scale_max].  sp: a SimParams (sim_params()), None for the defaults.  The result dictionary of
        icp_trimmed() with trace_sim (one {m, k, tau, kept, s_k, s_acc} row per traced pass) and sim_info (the last pass's) in
        place of the trimmed records, plus scale = sim_info[5] (1 when no pass ran); T holds the accumulated similarity."""
        out = self._pair(_SIM, src, tgt, None, None, params, _structs(_SIM, (sp,)), trace_cap, fitness_corr)
        out["scale"] = float(out["sim_info"][5]) if out["sim_info"][5] > 0 else 1.0
        return out

    def icp_sim_dev(self, d_src, ns, d_tgt, nt, params, sp=None):
        """kss_icp_sim_dev on device pointers; returns (IcpResult, sim_info)."""
        res = IcpResult()
        sp = sp if sp is not None else sim_params()
        info = np.zeros(SIM_NINFO, np.float64)
        self._chk(self.L.kss_icp_sim_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt), C.byref(params),
                                         C.byref(sp), C.byref(res), _p(info)), "kss_icp_sim_dev")
        return res, info

    # ---- robust ICP
    def robust_sums(self, src, tgt, normals, idx, max_d2=1.0, rp=None, loss=LOSS_HUBER, metric=METRIC_POINT):
        """kss_robust_sums: (sums, info) of one robust pass over given correspondences.  rp: a RobustParams (robust_params()), or
        None for the defaults of loss / metric.  normals: nt x 3 for the plane metric, None for the point metric; sums holds
        NSUMS or P2L_NSUMS doubles by metric, info {m, c2, sum of weights, cnt}."""
        rp, = _structs(_ROBUST, (rp,), loss, metric)
        s, t = _f32(src), _f32(tgt)
        nr = _f32(normals) if normals is not None else None
        i = np.ascontiguousarray(idx, dtype=np.int32)
        return self._sums(_ROBUST, False, (_p(s), _p(t), _p(nr), _p(i), len(s), len(t), float(max_d2)), (rp,),
                          P2L_NSUMS if rp.metric == METRIC_PLANE else NSUMS, True)

    def robust_sums_dev(self, d_src, d_tgt, d_normals, d_idx, n, nt, max_d2=1.0, rp=None, loss=LOSS_HUBER, metric=METRIC_POINT):
        """kss_robust_sums_dev on device pointers (d_normals 0 / None for the point metric); returns (sums, info)."""
        rp, = _structs(_ROBUST, (rp,), loss, metric)
        return self._sums(_ROBUST, True, (_dp(d_src), _dp(d_tgt), _dp(d_normals), _dp(d_idx), int(n), int(nt), float(max_d2)), (rp,),
                          P2L_NSUMS if rp.metric == METRIC_PLANE else NSUMS, True)

    def icp_robust(self, src, tgt, normals=None, rp=None, loss=LOSS_HUBER, metric=METRIC_POINT, params=None, trace_cap=0,
                   fitness_corr=False):
        """Robust ICP (kss_icp_robust): every pass weighs its correspondences with the loss's M-estimator weight, the scale
        fixed or taken per pass from the median residual.  rp: a RobustParams (robust_params()), or None for the defaults of
        loss / metric; normals as in icp_trimmed().  The result dictionary of icp_trimmed() with trace_robust (one {m, c2, sum
        of weights, cnt} row per traced pass) and robust_info (the last pass's) in place of the trimmed records."""
        return self._pair(_ROBUST, src, tgt, None, normals, params, _structs(_ROBUST, (rp,), loss, metric), trace_cap, fitness_corr)

    def icp_robust_dev(self, d_src, ns, d_tgt, nt, d_normals, params, rp=None, loss=LOSS_HUBER, metric=METRIC_POINT):
        """kss_icp_robust_dev on device pointers (d_normals may be 0 / None); returns (IcpResult, robust_info)."""
        rp = rp if rp is not None else robust_params(loss, metric)
        res = IcpResult()
        info = np.zeros(ROBUST_NINFO, np.float64)
        self._chk(self.L.kss_icp_robust_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                            C.c_void_p(int(d_normals)) if d_normals else None, C.byref(params), C.byref(rp),
                                            C.byref(res), _p(info)), "kss_icp_robust_dev")
        return res, info

    # ---- generalized ICP
    def gicp_sums(self, src, src_normals, tgt, tgt_normals, idx, max_d2=1.0, Rn=None, gp=None):
        """kss_gicp_sums: the P2L_NSUMS record of one generalized-ICP pass over given correspondences.  Rn: the 3 x 3 applied to the
        source normals (None: identity); either set of normals may be None (computed); gp: a GicpParams (gicp_params())."""
        return self._sums_both(_GICP, src, src_normals, tgt, tgt_normals, idx, max_d2, Rn, _structs(_GICP, (gp,)))

    def gicp_sums_dev(self, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2=1.0, Rn=None, gp=None):
        """kss_gicp_sums_dev on device pointers (either normals pointer may be 0 / None; Rn stays a host array)."""
        return self._sums_both_dev(_GICP, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2, Rn, _structs(_GICP, (gp,)))

    def icp_gicp(self, src, tgt, src_normals=None, tgt_normals=None, gp=None, params=None, trace_cap=0, fitness_corr=False):
        """Generalized ICP (kss_icp_gicp): every correspondence is weighed by the inverse of the sum of both points' surface
        covariances, given as the normals of both clouds (ns x 3 and nt x 3; None: computed with kss_normals' definition at
        gp.normals_k and rounded to float).  gp: a GicpParams (gicp_params()).  The result dictionary of icp_p2l()."""
        return self._pair(_GICP, src, tgt, src_normals, tgt_normals, params, _structs(_GICP, (gp,)), trace_cap, fitness_corr)

    def icp_gicp_dev(self, d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals, params, gp=None):
        """kss_icp_gicp_dev on device pointers (either normals pointer may be 0 / None); returns the IcpResult."""
        gp = gp if gp is not None else gicp_params()
        res = IcpResult()
        self._chk(self.L.kss_icp_gicp_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_src_normals)) if d_src_normals else None,
                                          C.c_void_p(int(d_tgt)), int(nt), C.c_void_p(int(d_tgt_normals)) if d_tgt_normals else None,
                                          C.byref(params), C.byref(gp), C.byref(res)), "kss_icp_gicp_dev")
        return res

    # ---- voxelized generalized ICP against a voxel map
    def vmap(self, tgt, leaf, normals=None, normals_k=20):
        """kss_vmap_create: the VoxelMap of the target (nt x 3) at voxel edge `leaf`; normals: nt x 3, or None to compute them at
        normals_k as icp_gicp does."""
        t = _f32(tgt)
        tn = _normals(normals, len(t), "target")
        vp = vmap_params(leaf=float(leaf), normals_k=int(normals_k))
        h = C.c_void_p()
        self._chk(self.L.kss_vmap_create(self.h, _p(t), len(t), _p(tn), C.byref(vp), C.byref(h)), "kss_vmap_create")
        return VoxelMap(self, h)

    def vmap_dev(self, d_tgt, nt, leaf, d_normals=None, normals_k=20):
        """kss_vmap_create_dev on device pointers (the normals pointer may be 0 / None)."""
        vp = vmap_params(leaf=float(leaf), normals_k=int(normals_k))
        h = C.c_void_p()
        self._chk(self.L.kss_vmap_create_dev(self.h, _dp(d_tgt), int(nt), _dp(d_normals), C.byref(vp), C.byref(h)), "kss_vmap_create_dev")
        return VoxelMap(self, h)

    def vgicp_sums(self, src, src_normals, vmap, max_d2=1.0, Rn=None, gp=None):
        """kss_vgicp_sums: the P2L_NSUMS record of one voxelized generalized-ICP pass at the positions passed in.  Rn: the 3 x 3
        applied to the source normals (None: identity); src_normals may be None (computed); gp: a GicpParams (gicp_params())."""
        s = _f32(src)
        sn = _normals(src_normals, len(s), "source")
        return self._sums(_VGICP, False, (_p(s), _p(sn), len(s), vmap.h if vmap is not None else None, float(max_d2), _p(_rot(Rn))),
                          _structs(_VGICP, (gp,)))

    def vgicp_sums_dev(self, d_src, d_src_normals, n, vmap, max_d2=1.0, Rn=None, gp=None):
        """kss_vgicp_sums_dev on device pointers (the normals pointer may be 0 / None; Rn stays a host array)."""
        return self._sums(_VGICP, True, (_dp(d_src), _dp(d_src_normals), int(n), vmap.h, float(max_d2), _p(_rot(Rn))),
                          _structs(_VGICP, (gp,)))

    def icp_vgicp(self, src, vmap, src_normals=None, gp=None, params=None, trace_cap=0):
        """Voxelized generalized ICP (kss_icp_vgicp) of the source (ns x 3) against a VoxelMap: icp_gicp's metric with the voxel's
        mean and average n n^T in the target's place, and no nearest-neighbour search.  src_normals: ns x 3, or None (computed at
        gp.normals_k).  The result dictionary of icp_gicp() plus "info", the VGICP_NINFO doubles {kept in the last pass, ns, [30]
        of the last pass, voxels}.  "fitness" is the mean squared distance to the voxel mean over the sources kept at the final
        pose, not icp()'s."""
        s = _f32(src)
        sn = _normals(src_normals, len(s), "source")
        p = params if params is not None else self.icp_params()
        return self._result(_VGICP, *self._icp_call(_VGICP, False, src=_p(s), ns=len(s), sn=_p(sn), tgt=vmap.h if vmap is not None else None,
                                                    nt=None, tn=None, p=p, structs=_structs(_VGICP, (gp,)), trace_cap=trace_cap))

    def icp_vgicp_dev(self, d_src, ns, d_src_normals, vmap, params, gp=None):
        """kss_icp_vgicp_dev on device pointers (the normals pointer may be 0 / None); returns (IcpResult, info)."""
        gp = gp if gp is not None else gicp_params()
        res = IcpResult()
        info = np.zeros(VGICP_NINFO, np.float64)
        self._chk(self.L.kss_icp_vgicp_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_src_normals)) if d_src_normals else None,
                                           vmap.h, C.byref(params), C.byref(gp), C.byref(res), _p(info)), "kss_icp_vgicp_dev")
        return res, info

    # ---- symmetric ICP
    def symm_sums(self, src, src_normals, tgt, tgt_normals, idx, max_d2=1.0, Rn=None, sp=None):
        """kss_symm_sums: the P2L_NSUMS record of one symmetric-ICP pass over given correspondences.  Rn: the 3 x 3 applied to the
        source normals (None: identity); either set of normals may be None (computed); sp: a SymmParams (symm_params())."""
        return self._sums_both(_SYMM, src, src_normals, tgt, tgt_normals, idx, max_d2, Rn, _structs(_SYMM, (sp,)))

    def symm_sums_dev(self, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2=1.0, Rn=None, sp=None):
        """kss_symm_sums_dev on device pointers (either normals pointer may be 0 / None; Rn stays a host array)."""
        return self._sums_both_dev(_SYMM, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2, Rn, _structs(_SYMM, (sp,)))

    def icp_symm(self, src, tgt, src_normals=None, tgt_normals=None, sp=None, params=None, trace_cap=0, fitness_corr=False):
        """Symmetric ICP (kss_icp_symm): the point-to-plane residual against the sum of both clouds' normals, each cloud turned by
        half the step (ns x 3 and nt x 3 normals; None: computed with kss_normals' definition at sp.normals_k and rounded to
        float).  sp: a SymmParams (symm_params()).  The result dictionary of icp_p2l()."""
        return self._pair(_SYMM, src, tgt, src_normals, tgt_normals, params, _structs(_SYMM, (sp,)), trace_cap, fitness_corr)

    def icp_symm_dev(self, d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals, params, sp=None):
        """kss_icp_symm_dev on device pointers (either normals pointer may be 0 / None); returns the IcpResult."""
        sp = sp if sp is not None else symm_params()
        res = IcpResult()
        self._chk(self.L.kss_icp_symm_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_src_normals)) if d_src_normals else None,
                                          C.c_void_p(int(d_tgt)), int(nt), C.c_void_p(int(d_tgt_normals)) if d_tgt_normals else None,
                                          C.byref(params), C.byref(sp), C.byref(res)), "kss_icp_symm_dev")
        return res

    # ---- robust symmetric ICP
    def symm_robust_sums(self, src, src_normals, tgt, tgt_normals, idx, max_d2=1.0, Rn=None, sp=None, rp=None, loss=LOSS_TUKEY):
        """kss_symm_robust_sums: (sums, info) of one robust symmetric pass over given correspondences: symm_sums()' arguments and a
        RobustParams of the plane metric (rp None: the defaults of loss).  sums holds P2L_NSUMS doubles in the robust plane layout,
        info {m, c2, sum of weights, cnt}."""
        return self._sums_both(_SYMM_ROBUST, src, src_normals, tgt, tgt_normals, idx, max_d2, Rn, _structs(_SYMM_ROBUST, (sp, rp), loss),
                               True)

    def symm_robust_sums_dev(self, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2=1.0, Rn=None, sp=None, rp=None,
                             loss=LOSS_TUKEY):
        """kss_symm_robust_sums_dev on device pointers (either normals pointer may be 0 / None; Rn stays a host array); returns
        (sums, info)."""
        return self._sums_both_dev(_SYMM_ROBUST, d_src, d_src_normals, d_tgt, d_tgt_normals, d_idx, n, nt, max_d2, Rn,
                                   _structs(_SYMM_ROBUST, (sp, rp), loss), True)

    def icp_symm_robust(self, src, tgt, src_normals=None, tgt_normals=None, sp=None, rp=None, loss=LOSS_TUKEY, params=None, trace_cap=0,
                        fitness_corr=False):
        """Robust symmetric ICP (kss_icp_symm_robust): icp_symm()'s metric with icp_robust()'s M-estimator weights, for pairs far
        apart in angle that carry outliers or overlap in part.  Normals and sp as in icp_symm(); rp: a RobustParams of the plane
        metric (None: the defaults of loss).  The result dictionary of icp_robust(), trace_robust and robust_info included."""
        return self._pair(_SYMM_ROBUST, src, tgt, src_normals, tgt_normals, params, _structs(_SYMM_ROBUST, (sp, rp), loss), trace_cap,
                          fitness_corr)

    def icp_symm_robust_dev(self, d_src, ns, d_src_normals, d_tgt, nt, d_tgt_normals, params, sp=None, rp=None, loss=LOSS_TUKEY):
        """kss_icp_symm_robust_dev on device pointers (either normals pointer may be 0 / None); returns (IcpResult, robust_info)."""
        sp = sp if sp is not None else symm_params()
        rp = rp if rp is not None else robust_params(loss, METRIC_PLANE)
        res = IcpResult()
        info = np.zeros(ROBUST_NINFO, np.float64)
        self._chk(self.L.kss_icp_symm_robust_dev(self.h, C.c_void_p(int(d_src)), int(ns),
                                                 C.c_void_p(int(d_src_normals)) if d_src_normals else None, C.c_void_p(int(d_tgt)), int(nt),
                                                 C.c_void_p(int(d_tgt_normals)) if d_tgt_normals else None, C.byref(params), C.byref(sp),
                                                 C.byref(rp), C.byref(res), _p(info)), "kss_icp_symm_robust_dev")
        return res, info

    # ---- point-to-plane and trimmed ICP, many pairs per call
    def icp_p2l_batch(self, src_all, src_off, tgt_all, tgt_off, normals_all=None, params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_p2l_batch: point-to-plane ICP of npairs pairs in one call (packed clouds, npairs + 1 offsets in points; normals_all
        laid out like tgt_all, or None to have them computed).  Returns (list of IcpResult, dictionary with pair 0's trace_sums /
        trace_Tk / fitness_idx / fitness_d2 where asked for)."""
        return self._pairs(_P2L, src_all, src_off, tgt_all, tgt_off, None, normals_all, params, (), (), trace_cap, fitness_corr)

    def icp_p2l_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, d_normals_all, params):
        """kss_icp_p2l_batch_dev on device pointers (d_normals_all may be 0 / None); returns the list of IcpResult."""
        so, to = self._offsets(src_off, tgt_off)
        res = (IcpResult * (len(so) - 1))()
        self._chk(self.L.kss_icp_p2l_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                               C.c_void_p(int(d_normals_all)) if d_normals_all else None, len(so) - 1, C.byref(params),
                                               C.cast(res, C.c_void_p)), "kss_icp_p2l_batch_dev")
        return list(res)

    def icp_trimmed_batch(self, src_all, src_off, tgt_all, tgt_off, normals_all=None, overlaps=None, overlap=0.5, metric=METRIC_POINT,
                          params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_trimmed_batch: trimmed ICP of npairs pairs in one call.  overlaps: one per pair, or None for `overlap` everywhere.
        Returns (list of IcpResult, trim_info of every pair as npairs x TRIM_NINFO, dictionary with pair 0's traces)."""
        return self._pairs(_TRIMMED, src_all, src_off, tgt_all, tgt_off, None, normals_all, params,
                           (TrimParams(float(overlap), int(metric), None),), (overlaps,), trace_cap, fitness_corr)

    def icp_trimmed_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, d_normals_all, params, overlaps=None, overlap=0.5,
                              metric=METRIC_POINT):
        """kss_icp_trimmed_batch_dev on device pointers; returns (list of IcpResult, trim_info npairs x TRIM_NINFO)."""
        so, to = self._offsets(src_off, tgt_off)
        npairs = len(so) - 1
        ov = _per_pair(overlaps, np.float64, npairs, "overlaps")
        res = (IcpResult * npairs)()
        tp = TrimParams(float(overlap), int(metric), None)
        info = np.zeros((npairs, TRIM_NINFO), np.float64)
        self._chk(self.L.kss_icp_trimmed_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                                   C.c_void_p(int(d_normals_all)) if d_normals_all else None, npairs, C.byref(params),
                                                   C.byref(tp), _p(ov), C.cast(res, C.c_void_p), _p(info)), "kss_icp_trimmed_batch_dev")
        return list(res), info

    def icp_o2o_batch(self, src_all, src_off, tgt_all, tgt_off, normals_all=None, overlaps=None, overlap=1.0, metric=METRIC_POINT,
                      params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_o2o_batch: one-to-one ICP of npairs pairs in one call.  Arguments as icp_trimmed_batch().  Returns (list of
        IcpResult, o2o_info of every pair as npairs x O2O_NINFO, dictionary with pair 0's traces)."""
        return self._pairs(_O2O, src_all, src_off, tgt_all, tgt_off, None, normals_all, params, (O2oParams(float(overlap), int(metric), None),),
                           (overlaps,), trace_cap, fitness_corr)

    def icp_o2o_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, d_normals_all, params, overlaps=None, overlap=1.0,
                          metric=METRIC_POINT):
        """kss_icp_o2o_batch_dev on device pointers; returns (list of IcpResult, o2o_info npairs x O2O_NINFO)."""
        so, to = self._offsets(src_off, tgt_off)
        npairs = len(so) - 1
        ov = _per_pair(overlaps, np.float64, npairs, "overlaps")
        res = (IcpResult * npairs)()
        op = O2oParams(float(overlap), int(metric), None)
        info = np.zeros((npairs, O2O_NINFO), np.float64)
        self._chk(self.L.kss_icp_o2o_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                               C.c_void_p(int(d_normals_all)) if d_normals_all else None, npairs, C.byref(params),
                                               C.byref(op), _p(ov), C.cast(res, C.c_void_p), _p(info)), "kss_icp_o2o_batch_dev")
        return list(res), info

    # ---- reciprocal ICP, many pairs per call (the C symbols of the loop are spelled _pairs: include/kssicp.h)
    def recip_filter_batch(self, src_all, off, tgt_all, tgt_off, idx_all, d2_all, max_d2=1.0, nn_fma=0):
        """kss_recip_filter_batch: the reciprocal filter of every segment -- sources [off[i], off[i + 1]) of src_all / idx_all / d2_all
        against targets [tgt_off[i], tgt_off[i + 1]) of tgt_all -- in one call.  Returns (idx_f, d2_f, info nseg x 3 = {m, u, r});
        entries outside the segments are left as given."""
        s, t = _f32(src_all), _f32(tgt_all)
        i = np.array(idx_all, dtype=np.int32).reshape(-1)
        d = np.array(d2_all, dtype=np.float32).reshape(-1)
        if len(i) != len(d) or len(i) != len(s):
            raise ValueError("idx and d2 must have one entry per source")
        o, to = self._offsets(off, tgt_off)
        nseg = len(o) - 1
        io, do = i.copy(), d.copy()
        info = np.zeros((max(nseg, 0), 3), np.float64)
        self._chk(self.L.kss_recip_filter_batch(self.h, _p(s), _p(o), _p(t), _p(to), nseg, _p(i), _p(d), float(max_d2), int(nn_fma), _p(io),
                                                _p(do), _p(info)), "kss_recip_filter_batch")
        return io, do, info

    def recip_filter_batch_dev(self, d_src_all, off, d_tgt_all, tgt_off, d_idx_all, d_d2_all, max_d2=1.0, nn_fma=0, d_idx_out_all=None,
                               d_d2_out_all=None):
        """kss_recip_filter_batch_dev on device pointers (an output may be 0 / None, or its input); returns info nseg x 3 = {m, u, r}."""
        o, to = self._offsets(off, tgt_off)
        nseg = len(o) - 1
        info = np.zeros((max(nseg, 0), 3), np.float64)
        self._chk(self.L.kss_recip_filter_batch_dev(self.h, _dp(d_src_all), _p(o), _dp(d_tgt_all), _p(to), nseg, _dp(d_idx_all),
                                                    _dp(d_d2_all), float(max_d2), int(nn_fma), _dp(d_idx_out_all), _dp(d_d2_out_all),
                                                    _p(info)), "kss_recip_filter_batch_dev")
        return info

    def icp_recip_batch(self, src_all, src_off, tgt_all, tgt_off, normals_all=None, overlaps=None, overlap=1.0, metric=METRIC_POINT,
                        params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_recip_pairs: reciprocal ICP of npairs pairs in one call.  Arguments as icp_o2o_batch().  Returns (list of
        IcpResult, recip_info of every pair as npairs x RECIP_NINFO, dictionary with pair 0's traces, trace_recip among them)."""
        return self._pairs(_RECIP, src_all, src_off, tgt_all, tgt_off, None, normals_all, params,
                           (RecipParams(float(overlap), int(metric), None),), (overlaps,), trace_cap, fitness_corr)

    def icp_recip_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, d_normals_all, params, overlaps=None, overlap=1.0,
                            metric=METRIC_POINT):
        """kss_icp_recip_pairs_dev on device pointers; returns (list of IcpResult, recip_info npairs x RECIP_NINFO)."""
        so, to = self._offsets(src_off, tgt_off)
        npairs = len(so) - 1
        ov = _per_pair(overlaps, np.float64, npairs, "overlaps")
        res = (IcpResult * npairs)()
        rp = RecipParams(float(overlap), int(metric), None)
        info = np.zeros((npairs, RECIP_NINFO), np.float64)
        self._chk(self.L.kss_icp_recip_pairs_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                                 C.c_void_p(int(d_normals_all)) if d_normals_all else None, npairs, C.byref(params),
                                                 C.byref(rp), _p(ov), C.cast(res, C.c_void_p), _p(info)), "kss_icp_recip_pairs_dev")
        return list(res), info

    def icp_sim_batch(self, src_all, src_off, tgt_all, tgt_off, overlaps=None, sp=None, params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_sim_batch: similarity ICP of npairs pairs in one call.  overlaps: one per pair, or None for sp.overlap everywhere.
        Returns (list of IcpResult, sim_info of every pair as npairs x SIM_NINFO -- column 5 is the pair's scale --, dictionary with
        pair 0's traces)."""
        return self._pairs(_SIM, src_all, src_off, tgt_all, tgt_off, None, None, params, _structs(_SIM, (sp,)), (overlaps,), trace_cap,
                           fitness_corr)

    def icp_sim_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, params, overlaps=None, sp=None):
        """kss_icp_sim_batch_dev on device pointers; returns (list of IcpResult, sim_info npairs x SIM_NINFO)."""
        so, to = self._offsets(src_off, tgt_off)
        npairs = len(so) - 1
        ov = _per_pair(overlaps, np.float64, npairs, "overlaps")
        res = (IcpResult * npairs)()
        sp = sp if sp is not None else sim_params()
        info = np.zeros((npairs, SIM_NINFO), np.float64)
        self._chk(self.L.kss_icp_sim_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to), npairs,
                                               C.byref(params), C.byref(sp), _p(ov), C.cast(res, C.c_void_p), _p(info)),
                  "kss_icp_sim_batch_dev")
        return list(res), info

    # ---- robust ICP, many pairs per call
    def icp_robust_batch(self, src_all, src_off, tgt_all, tgt_off, normals_all=None, rp=None, loss=LOSS_HUBER, metric=METRIC_POINT,
                         scales=None, params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_robust_batch: robust ICP of npairs pairs in one call.  rp as in icp_robust() (loss, metric, tune and min_scale of
        the whole batch); scales: one per pair (> 0 fixed, 0 automatic), or None for rp.scale everywhere.  Returns (list of
        IcpResult, robust_info of every pair as npairs x ROBUST_NINFO, dictionary with pair 0's traces, trace_robust among them)."""
        return self._pairs(_ROBUST, src_all, src_off, tgt_all, tgt_off, None, normals_all, params,
                           _structs(_ROBUST, (rp,), loss, metric), (scales,), trace_cap, fitness_corr)

    def icp_robust_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, d_normals_all, params, rp=None, loss=LOSS_HUBER,
                             metric=METRIC_POINT, scales=None):
        """kss_icp_robust_batch_dev on device pointers; returns (list of IcpResult, robust_info npairs x ROBUST_NINFO)."""
        rp = rp if rp is not None else robust_params(loss, metric)
        so, to = self._offsets(src_off, tgt_off)
        npairs = len(so) - 1
        sc = _per_pair(scales, np.float64, npairs, "scales")
        res = (IcpResult * npairs)()
        info = np.zeros((npairs, ROBUST_NINFO), np.float64)
        self._chk(self.L.kss_icp_robust_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                                  C.c_void_p(int(d_normals_all)) if d_normals_all else None, npairs, C.byref(params),
                                                  C.byref(rp), _p(sc), C.cast(res, C.c_void_p), _p(info)), "kss_icp_robust_batch_dev")
        return list(res), info

    # ---- generalized ICP, many pairs per call
    def icp_gicp_batch(self, src_all, src_off, tgt_all, tgt_off, src_normals_all=None, tgt_normals_all=None, epsilons=None, gp=None,
                       params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_gicp_batch: generalized ICP of npairs pairs in one call (packed clouds, npairs + 1 offsets in points; the normals
        laid out like their clouds, either None to have them computed per cloud at gp.normals_k).  epsilons: one per pair, or None
        for gp.epsilon everywhere.  Returns (list of IcpResult, dictionary with pair 0's trace_sums / trace_Tk / fitness_idx /
        fitness_d2 where asked for)."""
        return self._pairs(_GICP, src_all, src_off, tgt_all, tgt_off, src_normals_all, tgt_normals_all, params, _structs(_GICP, (gp,)),
                           (epsilons,), trace_cap, fitness_corr)

    def icp_gicp_batch_dev(self, d_src_all, src_off, d_src_normals_all, d_tgt_all, tgt_off, d_tgt_normals_all, params=None, epsilons=None,
                           gp=None, trace_cap=0):
        """kss_icp_gicp_batch_dev on device pointers (either normals pointer may be 0 / None; the offsets stay host arrays).
        Returns (list of IcpResult, dictionary with pair 0's trace_sums / trace_Tk where asked for)."""
        return self._pairs_dev_traced(_GICP, d_src_all, src_off, d_tgt_all, tgt_off, d_src_normals_all, d_tgt_normals_all, params,
                               _structs(_GICP, (gp,)), (epsilons,), trace_cap)

    # ---- symmetric ICP, many pairs per call
    def icp_symm_batch(self, src_all, src_off, tgt_all, tgt_off, src_normals_all=None, tgt_normals_all=None, aligns=None, sp=None,
                       params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_symm_batch: symmetric ICP of npairs pairs in one call (packed clouds, npairs + 1 offsets in points; the normals
        laid out like their clouds, either None to have them computed per cloud at sp.normals_k).  aligns: one align_normals (0 or
        1) per pair, or None for sp.align_normals everywhere.  Returns (list of IcpResult, dictionary with pair 0's trace_sums /
        trace_Tk / fitness_idx / fitness_d2 where asked for)."""
        return self._pairs(_SYMM, src_all, src_off, tgt_all, tgt_off, src_normals_all, tgt_normals_all, params, _structs(_SYMM, (sp,)),
                           (aligns,), trace_cap, fitness_corr)

    def icp_symm_batch_dev(self, d_src_all, src_off, d_src_normals_all, d_tgt_all, tgt_off, d_tgt_normals_all, params=None, aligns=None,
                           sp=None, trace_cap=0):
        """kss_icp_symm_batch_dev on device pointers (either normals pointer may be 0 / None; the offsets and aligns stay host
        arrays).  Returns (list of IcpResult, dictionary with pair 0's trace_sums / trace_Tk where asked for)."""
        return self._pairs_dev_traced(_SYMM, d_src_all, src_off, d_tgt_all, tgt_off, d_src_normals_all, d_tgt_normals_all, params,
                               _structs(_SYMM, (sp,)), (aligns,), trace_cap)

    # ---- robust symmetric ICP, many pairs per call
    def icp_symm_robust_batch(self, src_all, src_off, tgt_all, tgt_off, src_normals_all=None, tgt_normals_all=None, aligns=None,
                              scales=None, sp=None, rp=None, loss=LOSS_TUKEY, params=None, trace_cap=0, fitness_corr=False):
        """kss_icp_symm_robust_batch: robust symmetric ICP of npairs pairs in one call.  Clouds, offsets, normals, aligns and sp as in
        icp_symm_batch(); rp as in icp_symm_robust() (loss, tune and min_scale of the whole batch); scales: one per pair (> 0 fixed,
        0 automatic), or None for rp.scale everywhere.  Returns (list of IcpResult, robust_info of every pair as npairs x
        ROBUST_NINFO, dictionary with pair 0's traces, trace_robust among them)."""
        return self._pairs(_SYMM_ROBUST, src_all, src_off, tgt_all, tgt_off, src_normals_all, tgt_normals_all, params,
                           _structs(_SYMM_ROBUST, (sp, rp), loss), (aligns, scales), trace_cap, fitness_corr)

    def icp_symm_robust_batch_dev(self, d_src_all, src_off, d_src_normals_all, d_tgt_all, tgt_off, d_tgt_normals_all, params=None,
                                  aligns=None, scales=None, sp=None, rp=None, loss=LOSS_TUKEY, trace_cap=0):
        """kss_icp_symm_robust_batch_dev on device pointers (either normals pointer may be 0 / None; the offsets, aligns and scales
        stay host arrays).  Returns (list of IcpResult, robust_info npairs x ROBUST_NINFO, dictionary with pair 0's traces)."""
        return self._pairs_dev_traced(_SYMM_ROBUST, d_src_all, src_off, d_tgt_all, tgt_off, d_src_normals_all,
                               d_tgt_normals_all, params, _structs(_SYMM_ROBUST, (sp, rp), loss), (aligns, scales), trace_cap)

    def trim_threshold_batch(self, d2_all, off, overlaps, max_d2=1.0):
        """kss_trim_threshold_batch: {m, k, tau, kept} of every segment [off[i], off[i + 1]) of d2_all, nseg x TRIM_NINFO."""
        d = np.ascontiguousarray(d2_all, dtype=np.float32).reshape(-1)
        o = np.ascontiguousarray(off, dtype=np.int64)
        ov = _per_pair(overlaps, np.float64, len(o) - 1, "overlaps")
        info = np.zeros((max(len(o) - 1, 0), TRIM_NINFO), np.float64)
        self._chk(self.L.kss_trim_threshold_batch(self.h, _p(d), _p(o), len(o) - 1, float(max_d2), _p(ov), _p(info)), "kss_trim_threshold_batch")
        return info

    def trim_threshold_batch_dev(self, d_d2_all, off, overlaps, max_d2=1.0):
        o = np.ascontiguousarray(off, dtype=np.int64)
        ov = _per_pair(overlaps, np.float64, len(o) - 1, "overlaps")
        info = np.zeros((max(len(o) - 1, 0), TRIM_NINFO), np.float64)
        self._chk(self.L.kss_trim_threshold_batch_dev(self.h, _dp(d_d2_all), _p(o), len(o) - 1, float(max_d2), _p(ov), _p(info)),
                  "kss_trim_threshold_batch_dev")
        return info

    def icp_dev(self, d_src, ns, d_tgt, nt, params):
        res = IcpResult()
        self._chk(self.L.kss_icp_dev(self.h, C.c_void_p(int(d_src)), int(ns), C.c_void_p(int(d_tgt)), int(nt),
                                     C.byref(params), C.byref(res)), "kss_icp_dev")
        return res

    def icp_batch(self, src_all, src_off, tgt_all, tgt_off, params=None):
        s, t = _f32(src_all), _f32(tgt_all)
        so = np.ascontiguousarray(src_off, dtype=np.int64)
        to = np.ascontiguousarray(tgt_off, dtype=np.int64)
        npairs = len(so) - 1
        p = params if params is not None else self.icp_params()
        res = (IcpResult * npairs)()
        self._chk(self.L.kss_icp_batch(self.h, _p(s), _p(so), _p(t), _p(to), npairs, C.byref(p), C.cast(res, C.c_void_p)), "kss_icp_batch")
        return list(res)

    def icp_batch_dev(self, d_src_all, src_off, d_tgt_all, tgt_off, params):
        so = np.ascontiguousarray(src_off, dtype=np.int64)
        to = np.ascontiguousarray(tgt_off, dtype=np.int64)
        npairs = len(so) - 1
        res = (IcpResult * npairs)()
        self._chk(self.L.kss_icp_batch_dev(self.h, C.c_void_p(int(d_src_all)), _p(so), C.c_void_p(int(d_tgt_all)), _p(to),
                                           npairs, C.byref(params), C.cast(res, C.c_void_p)), "kss_icp_batch_dev")
        return res

    # ---- voxelized generalized ICP, many scans against one map per call
    def icp_vgicp_batch(self, src_all, src_off, vmap, src_normals_all=None, epsilons=None, gp=None, params=None, trace_cap=0):
        """kss_icp_vgicp_batch: voxelized generalized ICP of nscans scans (packed, nscans + 1 offsets in points) against ONE
        VoxelMap in one call.  src_normals_all: laid out like src_all, or None to have every scan's computed at gp.normals_k;
        epsilons: one per scan, or None for gp.epsilon everywhere.  Returns a list of icp_vgicp()'s dictionaries, one per scan
        ("info": the scan's VGICP_NINFO doubles, "pair_id": its index), scan 0's trace_sums / trace_Tk on entry 0 where asked for."""
        s = _f32(src_all)
        sn = _normals(src_normals_all, len(s), "source")
        so = np.ascontiguousarray(src_off, dtype=np.int64)
        p = params if params is not None else self.icp_params()
        res, info, extra = self._icp_call(_VGICP_BATCH, False, _p(s), _p(so), _p(sn), vmap.h if vmap is not None else None, None, None, p,
                                          _structs(_VGICP_BATCH, (gp,)), (epsilons,), so, trace_cap)
        return [dict(self._result(_VGICP_BATCH, r, info[i], extra if i == 0 else {}), pair_id=r.pair_id) for i, r in enumerate(res)]

    def vmap_box(self, lo, hi, leaf):
        """kss_vmap_create_box: an EMPTY VoxelMap over the box lo .. hi (3 floats each) at voxel edge `leaf`, to be filled by
        VoxelMap.insert()."""
        a = np.ascontiguousarray(lo, dtype=np.float32).reshape(3)
        b = np.ascontiguousarray(hi, dtype=np.float32).reshape(3)
        vp = vmap_params(leaf=float(leaf))
        h = C.c_void_p()
        self._chk(self.L.kss_vmap_create_box(self.h, _p(a), _p(b), C.byref(vp), C.byref(h)), "kss_vmap_create_box")
        return VoxelMap(self, h)

    def icp_vgicp_batch_dev(self, d_src_all, src_off, d_src_normals_all, vmap, params, epsilons=None, gp=None):
        """kss_icp_vgicp_batch_dev on device pointers (the normals pointer may be 0 / None; the offsets and epsilons stay host
        arrays); returns (list of IcpResult, info nscans x VGICP_NINFO)."""
        so = np.ascontiguousarray(src_off, dtype=np.int64)
        res, info, _ = self._icp_call(_VGICP_BATCH, True, _dp(d_src_all), _p(so), _dp(d_src_normals_all), vmap.h, None, None, params,
                                      _structs(_VGICP_BATCH, (gp,)), (epsilons,), so)
        return list(res), info

    # ---- voxelized generalized ICP from a start pose and coarse to fine (the pyramid)
    def _vgicp_traced(self, name, p, trace_cap, call, nlevels=None):
        """The checked call of a kss_icp_vgicp_from / _c2f entry with the caller's trace attached to p and detached again; returns
        the dictionary of the extras."""
        if trace_cap <= 0:
            self._chk(call(), name)
            return {}
        tr = (np.zeros((trace_cap, P2L_NSUMS), np.float64), np.zeros((trace_cap, 16), np.float32), C.c_int(0))
        try:
            p.trace_sums = tr[0].ctypes.data_as(C.POINTER(C.c_double))
            p.trace_Tk = tr[1].ctypes.data_as(C.POINTER(C.c_float))
            p.trace_cap = trace_cap
            p.trace_n = C.pointer(tr[2])
            self._chk(call(), name)
        finally:
            p.trace_sums = None; p.trace_Tk = None; p.trace_cap = 0; p.trace_n = None
        n = tr[2].value
        return {"trace_sums": tr[0][:n].copy(), "trace_Tk": tr[1][:n].reshape(-1, 4, 4).copy()}

    @staticmethod
    def _pose(T0):
        return None if T0 is None else np.ascontiguousarray(T0, dtype=np.float32).reshape(16)

    def icp_vgicp_from(self, src, vmap, T0, src_normals=None, gp=None, params=None, trace_cap=0):
        """kss_icp_vgicp_from: icp_vgicp() with the accumulated pose started at T0 (a 4 x 4; None: icp_vgicp itself).  The result's
        "T" includes T0; the normals are turned from the original ones in every pass."""
        s = _f32(src)
        sn = _normals(src_normals, len(s), "source")
        p = params if params is not None else self.icp_params()
        gp = gp if gp is not None else gicp_params()
        res, info, Tm = IcpResult(), np.zeros(VGICP_NINFO, np.float64), self._pose(T0)
        extra = self._vgicp_traced("kss_icp_vgicp_from", p, trace_cap, lambda: self.L.kss_icp_vgicp_from(
            self.h, _p(s), len(s), _p(sn), vmap.h if vmap is not None else None, _p(Tm), C.byref(p), C.byref(gp), C.byref(res), _p(info)))
        return self._result(_VGICP, res, info, extra)

    def icp_vgicp_from_dev(self, d_src, ns, d_src_normals, vmap, T0, params, gp=None):
        """kss_icp_vgicp_from_dev on device pointers (the normals pointer may be 0 / None; T0 stays a host array); returns
        (IcpResult, info)."""
        gp = gp if gp is not None else gicp_params()
        res, info, Tm = IcpResult(), np.zeros(VGICP_NINFO, np.float64), self._pose(T0)
        self._chk(self.L.kss_icp_vgicp_from_dev(self.h, _dp(d_src), int(ns), _dp(d_src_normals), vmap.h, _p(Tm), C.byref(params), C.byref(gp),
                                                C.byref(res), _p(info)), "kss_icp_vgicp_from_dev")
        return res, info

    @staticmethod
    def _levels(vmaps):
        return (C.c_void_p * len(vmaps))(*[m.h if m is not None else None for m in vmaps])

    def icp_vgicp_c2f(self, src, vmaps, T0=None, src_normals=None, gp=None, params=None, trace_cap=0):
        """kss_icp_vgicp_c2f: the ladder -- icp_vgicp_from() on every VoxelMap of vmaps in turn (the coarsest first), each level
        from the pose of the one before, the scan staged and its normals computed once.  Returns a list of icp_vgicp()'s
        dictionaries, one per level; "fitness" is evaluated and the trace filled for the last level only."""
        s = _f32(src)
        sn = _normals(src_normals, len(s), "source")
        p = params if params is not None else self.icp_params()
        gp = gp if gp is not None else gicp_params()
        n = len(vmaps)
        res, info, Tm, lv = (IcpResult * max(n, 1))(), np.zeros((max(n, 1), VGICP_NINFO), np.float64), self._pose(T0), self._levels(vmaps)
        extra = self._vgicp_traced("kss_icp_vgicp_c2f", p, trace_cap, lambda: self.L.kss_icp_vgicp_c2f(
            self.h, _p(s), len(s), _p(sn), C.cast(lv, C.c_void_p), n, _p(Tm), C.byref(p), C.byref(gp), C.cast(res, C.c_void_p), _p(info)))
        return [self._result(_VGICP, res[l], info[l], extra if l == n - 1 else {}) for l in range(n)]

    def icp_vgicp_c2f_dev(self, d_src, ns, d_src_normals, vmaps, T0, params, gp=None):
        """kss_icp_vgicp_c2f_dev on device pointers (the normals pointer may be 0 / None; T0 stays a host array or None); returns
        (list of IcpResult, info [nlevels, VGICP_NINFO])."""
        gp = gp if gp is not None else gicp_params()
        n = len(vmaps)
        res, info, Tm, lv = (IcpResult * max(n, 1))(), np.zeros((max(n, 1), VGICP_NINFO), np.float64), self._pose(T0), self._levels(vmaps)
        self._chk(self.L.kss_icp_vgicp_c2f_dev(self.h, _dp(d_src), int(ns), _dp(d_src_normals), C.cast(lv, C.c_void_p), n, _p(Tm),
                                               C.byref(params), C.byref(gp), C.cast(res, C.c_void_p), _p(info)), "kss_icp_vgicp_c2f_dev")
        return list(res)[:n], info[:n]

    def transform_apply_f32(self, T, pts):
        a = _f32(pts)
        Tm = np.ascontiguousarray(T, dtype=np.float32).reshape(16)
        out = np.empty_like(a)
        self._chk(self.L.kss_transform_apply_f32(self.h, _p(Tm), _p(a), len(a), _p(out)), "kss_transform_apply_f32")
        return out

    def downsample_fps(self, pts, m):
        a = _f64(pts)
        out = np.empty((int(m), 3), np.float64)
        idx = np.empty(int(m), np.int32)
        self._chk(self.L.kss_downsample_fps(self.h, _p(a), len(a), int(m), _p(out), _p(idx)), "kss_downsample_fps")
        return out, idx

    def downsample_aivs(self, pts, point_num):
        a = _f64(pts)
        out = np.empty_like(a)
        idx = np.empty(len(a), np.int32)
        k = C.c_int64(0)
        self._chk(self.L.kss_downsample_aivs(self.h, _p(a), len(a), int(point_num), _p(out), len(a), C.byref(k), _p(idx)), "kss_downsample_aivs")
        return out[:k.value].copy(), idx[:k.value].copy()

    def downsample_aivs_pair(self, pts0, point_num0, pts1, point_num1):
        """Both clouds of a registration at once (the second on a worker context): ((points, indices), (points, indices))."""
        a, b = _f64(pts0), _f64(pts1)
        oa, ob = np.empty_like(a), np.empty_like(b)
        ia, ib = np.empty(len(a), np.int32), np.empty(len(b), np.int32)
        ka, kb = C.c_int64(0), C.c_int64(0)
        rc = (C.c_int * 2)(0, 0)
        self._chk(self.L.kss_downsample_aivs_pair(self.h, _p(a), len(a), int(point_num0), _p(oa), len(a), C.byref(ka), _p(ia),
                                                  _p(b), len(b), int(point_num1), _p(ob), len(b), C.byref(kb), _p(ib), rc), "kss_downsample_aivs_pair")
        for k in range(2):
            self._chk(rc[k], "kss_downsample_aivs_pair (cloud %d)" % k)
        return (oa[:ka.value].copy(), ia[:ka.value].copy()), (ob[:kb.value].copy(), ib[:kb.value].copy())

    def normals_orient(self, pts, normals):
        a = _f64(pts); nrm = _f64(normals).copy()
        self._chk(self.L.kss_normals_orient(self.h, _p(a), len(a), _p(nrm)), "kss_normals_orient")
        return nrm

    def register_batch(self, src_all, src_off, tgt_all, tgt_off, sample_cap=2000, accurate=8.0, iters=1000, workers=0, want_align=False):
        s, t = _f64(src_all), _f64(tgt_all)
        so = np.ascontiguousarray(src_off, dtype=np.int64); to = np.ascontiguousarray(tgt_off, dtype=np.int64)
        npairs = len(so) - 1
        res = (RegisterResult * npairs)()
        align = np.empty_like(s) if want_align else None
        self._chk(self.L.kss_register_batch(self.h, _p(s), _p(so), _p(t), _p(to), npairs, int(sample_cap), float(accurate), int(iters),
                                            int(workers), _p(align) if want_align else None, C.cast(res, C.c_void_p)), "kss_register_batch")
        return (list(res), align) if want_align else list(res)

    def downsample_octree(self, pts):
        """(selected point indices in octree depth-first voxel order -- repeats possible --, resolution)."""
        a = _f64(pts)
        idx = np.empty(len(a), np.int32)
        k = C.c_int64(0)
        res = C.c_double(0)
        self._chk(self.L.kss_downsample_octree(self.h, _p(a), len(a), _p(idx), len(a), C.byref(k), C.byref(res)), "kss_downsample_octree")
        return idx[:k.value].copy(), res.value

    def knn(self, query, tgt, k):
        q, t = _f32(query), _f32(tgt)
        idx = np.empty((len(q), int(k)), np.int32)
        d2 = np.empty((len(q), int(k)), np.float32)
        self._chk(self.L.kss_knn(self.h, _p(q), len(q), _p(t), len(t), int(k), _p(idx), _p(d2)), "kss_knn")
        return idx, d2

    def normals(self, pts, k=20):
        a = _f64(pts)
        out = np.empty_like(a)
        self._chk(self.L.kss_normals(self.h, _p(a), len(a), int(k), _p(out)), "kss_normals")
        return out

    # ---- PCR_QM
    def pcr_qm(self, aligned, tmpl):
        a, t = _f64(aligned), _f64(tmpl)
        out = np.empty(3, np.float64)
        self._chk(self.L.kss_pcr_qm(self.h, _p(a), len(a), _p(t), len(t), _p(out)), "kss_pcr_qm")
        return out

    # ---- (a16)
    def register(self, src_sub, tgt_sub, src_full, accurate=8.0, iters=1000):
        s, t, f = _f64(src_sub), _f64(tgt_sub), _f64(src_full)
        align = np.empty_like(f)
        r = RegisterResult()
        self._chk(self.L.kss_register(self.h, _p(s), len(s), _p(t), len(t), _p(f), len(f), float(accurate), int(iters),
                                      _p(align), C.byref(r)), "kss_register")
        return {"pointAlign": align, "scale": r.scale, "angle": np.array(r.angle), "R": np.array(r.R).reshape(3, 3),
                "t": np.array(r.t), "T_icp": np.array(r.T_icp, dtype=np.float32).reshape(4, 4),
                "E_d_init": r.E_d_init, "final_fitness": r.final_fitness, "used_angle_list": bool(r.used_angle_list),
                "angle_index": r.angle_index, "n_angle_list": r.n_angle_list, "icp_iterations": r.icp_iterations,
                "icp_converged": bool(r.icp_converged), "grid": r.grid}
