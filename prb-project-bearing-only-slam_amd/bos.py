"""ctypes binding of libbos.so (include/bos.h, include/bos_host.h).

Python mirror of the reference's host interface for the GN path
(torchipeppo/prb-project-bearing-only-slam):

* :func:`load_g2o`  — ``parse_g2o`` + default fixed pose + ``triangulate_landmarks``
  (utils/g2o_utils.cpp:10-146, executables/bearing_only_slam.cpp:62-71,
  slam/triangulation.cpp:65-74), implemented in C++ inside libbos.so.
* :class:`Solver`   — ``proj02::Solver`` (slam/solver.hpp:21-92): ``step()``,
  ``set_kernel_threshold``, ``set_damping_factor``, ``state``.

There is no CPU fallback: constructing a :class:`Solver` without a visible HIP device raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libbos.so")
# diagnostics tools that load an older build (tools/gn_ab.py) set this: its missing entry points
# are then left unbound instead of failing the load
ALLOW_MISSING_SYMBOLS = False

BOS_OK = 0
BOS_FP64 = 64
BOS_FP32 = 32
BOS_SOLVER_SUPERNODAL = 0
BOS_SOLVER_DENSE_CHOL = 1
BOS_SOLVER_ROCSOLVER_RF = 2
BOS_SOLVER_SCHUR = 3
BOS_SOLVER_SPARSE_CHOL = BOS_SOLVER_SCHUR
BOS_PARTITION_SUBTREE = 0
BOS_PARTITION_OBSERVATIONS = 1
ABI_VERSION = 3

# every symbol declared in include/bos.h and include/bos_host.h
EXPORTED_SYMBOLS = [
    "bos_default_options", "bos_last_error", "bos_abi_version", "bos_device_count", "bos_device_peer_access",
    "bos_nccl_unique_id",
    "bos_create", "bos_destroy", "bos_set_kernel_threshold", "bos_set_damping_factor", "bos_step", "bos_step_n",
    "bos_linearize", "bos_linearize_async", "bos_synchronize", "bos_system_info_get", "bos_export_system",
    "bos_get_state", "bos_set_state", "bos_get_last_dx",
    "bos_dataset_load_g2o", "bos_dataset_synthetic", "bos_dataset_problem", "bos_dataset_pose_ids",
    "bos_dataset_landmark_ids", "bos_dataset_fixed_pose_id", "bos_dataset_bound", "bos_dataset_ground_truth",
    "bos_dataset_write_g2o", "bos_dataset_free", "bos_plan_inspect", "bos_plan_mf_selftest",
    "bos_debug_linearize_timeline", "bos_triangulate", "bos_triangulate_async", "bos_plan_shard_selftest",
    "bos_plan_node_owner", "bos_step_phase", "bos_exchange_size", "bos_exchange_download", "bos_exchange_upload",
    "bos_node_owner",
    "bos_debug_set_g2o_parser", "bos_debug_inject_stall", "bos_debug_set_step_graph", "bos_debug_solver_stamps",
    "bos_debug_solver_routes", "bos_debug_selinv_fronts", "bos_plan_mf_fronts",
    "bos_time_linearize", "bos_time_triangulate", "bos_time_steps", "bos_cpu_gn_create", "bos_cpu_gn_step", "bos_cpu_gn_get_state",
    "bos_cpu_gn_destroy", "bos_normalized_angle_f64", "bos_normalized_angle_f32", "bos_exchange_p2p_handle",
    "bos_exchange_p2p_connect", "bos_time_facade_steps", "bos_debug_facade_selftest", "bos_set_exchange_timeout",
    "bos_last_step_stamps", "bos_marginals", "bos_plan_mf_marginals", "bos_marginals_timing",
    "bos_lm_default_options", "bos_cost", "bos_optimize", "bos_time_cost", "bos_cpu_gn_set_kernel_threshold",
    "bos_cpu_gn_cost", "bos_cpu_gn_optimize", "bos_lm_rule_apply",
    "bos_edge_covariances", "bos_plan_mf_edge_covariances", "bos_edge_covariances_timing",
    "bos_edge_consistency", "bos_plan_mf_edge_consistency", "bos_edge_consistency_timing",
    "bos_pair_covariances", "bos_plan_mf_pair_covariances", "bos_plan_pair_paths", "bos_pair_covariances_timing",
    "bos_debug_set_pair_batch",
    "bos_node_covariances", "bos_plan_mf_node_covariances", "bos_node_covariances_timing",
    "bos_associate_bearings", "bos_plan_mf_associate_bearings", "bos_associate_bearings_timing",
    "bos_debug_set_associate_chunk", "bos_associate_tile",
    "bos_match_landmarks", "bos_match_poses", "bos_plan_mf_match_landmarks", "bos_plan_mf_match_poses",
    "bos_match_information_inverse", "bos_match_timing", "bos_debug_set_match_chunk",
    "bos_joint_compatibility", "bos_plan_mf_joint_compatibility", "bos_joint_compatibility_timing",
    "bos_debug_set_joint_batch",
    "bos_jcbb", "bos_jcbb_search_host", "bos_plan_mf_jcbb", "bos_jcbb_timing", "bos_debug_set_jcbb_batch",
    "bos_set_priors", "bos_cpu_gn_set_priors", "bos_prior_terms",
]

# bos_lm_result.reason
LM_STOP_DX, LM_STOP_COST, LM_STOP_ITERATIONS, LM_STOP_LAMBDA = 1, 2, 3, 4
LM_MAX_ITERATIONS = 4096

P2P_HANDLE_BYTES = 64   # include/bos.h BOS_P2P_HANDLE_BYTES

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
# the outputs of bos_edge_consistency: per kind the lists and the count, then the rows of both kinds
_EDGE_CHECK_SIG = [_ip, _dp, _dp, _dp, _ip] * 2 + [_dp] * 6


class BosError(RuntimeError):
    pass


class bos_problem(ctypes.Structure):
    _fields_ = [("num_poses", ctypes.c_int32), ("num_landmarks", ctypes.c_int32),
                ("num_bearings", ctypes.c_int32), ("num_odometry", ctypes.c_int32),
                ("pose_xyt", _dp), ("landmark_xy", _dp), ("bearing_pose", _ip), ("bearing_landmark", _ip),
                ("bearing_z", _dp), ("bearing_omega", _dp), ("odom_src", _ip), ("odom_dst", _ip),
                ("odom_z", _dp), ("odom_omega", _dp), ("fixed_pose", ctypes.c_int32)]


class bos_options(ctypes.Structure):
    _fields_ = [("precision", ctypes.c_int32), ("solver", ctypes.c_int32), ("device", ctypes.c_int32),
                ("rank", ctypes.c_int32), ("world_size", ctypes.c_int32), ("nccl_unique_id", ctypes.c_void_p),
                ("kernel_threshold", ctypes.c_double), ("damping", ctypes.c_double), ("stream", ctypes.c_void_p),
                ("partition", ctypes.c_int32), ("lanes_per_pose", ctypes.c_int32), ("schur_leaf", ctypes.c_int32)]


class bos_step_stats(ctypes.Structure):
    _fields_ = [("chi2", ctypes.c_double), ("n_robust", ctypes.c_int32), ("solver_info", ctypes.c_int32),
                ("max_abs_dx", ctypes.c_double), ("t_linearize_ms", ctypes.c_double),
                ("t_exchange_ms", ctypes.c_double), ("t_solve_ms", ctypes.c_double), ("t_update_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class bos_system_info(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("nnz_lower", ctypes.c_int64), ("nnz_factor", ctypes.c_int64),
                ("algorithmic_bytes", ctypes.c_int64), ("num_block_values", ctypes.c_int64),
                ("lanes_per_pose", ctypes.c_int32), ("pose_lane_groups", ctypes.c_int32),
                ("landmark_lanes", ctypes.c_int32), ("own_fronts", ctypes.c_int32), ("top_fronts", ctypes.c_int32),
                ("comm_ranks", ctypes.c_int32), ("partition", ctypes.c_int32),
                ("pl_factored", ctypes.c_int32), ("fold_fp32", ctypes.c_int32), ("layout_bytes", ctypes.c_int64)]


class bos_lm_options(ctypes.Structure):
    _fields_ = [("lambda0", ctypes.c_double), ("lambda_min", ctypes.c_double), ("lambda_max", ctypes.c_double),
                ("dx_tol", ctypes.c_double), ("f_tol", ctypes.c_double), ("max_iterations", ctypes.c_int32),
                ("check_every", ctypes.c_int32)]


class bos_lm_iteration(ctypes.Structure):
    _fields_ = [("cost", ctypes.c_double), ("cost_trial", ctypes.c_double), ("predicted", ctypes.c_double),
                ("gain", ctypes.c_double), ("lambda", ctypes.c_double), ("max_abs_dx", ctypes.c_double),
                ("solver_info", ctypes.c_int32), ("accepted", ctypes.c_int32)]


class bos_lm_result(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("accepted", ctypes.c_int32), ("rejected", ctypes.c_int32),
                ("reason", ctypes.c_int32), ("cost_initial", ctypes.c_double), ("cost_final", ctypes.c_double),
                ("lambda_final", ctypes.c_double)]


class bos_lm_state(ctypes.Structure):
    _fields_ = [("lambda", ctypes.c_double), ("nu", ctypes.c_double), ("cost", ctypes.c_double),
                ("iteration", ctypes.c_int32), ("accepted", ctypes.c_int32), ("rejected", ctypes.c_int32),
                ("done", ctypes.c_int32), ("reason", ctypes.c_int32)]


# one record of an optimize() trace (bos_lm_iteration)
LM_TRACE_DTYPE = np.dtype([("cost", "f8"), ("cost_trial", "f8"), ("predicted", "f8"), ("gain", "f8"), ("lambda", "f8"),
                           ("max_abs_dx", "f8"), ("solver_info", "i4"), ("accepted", "i4")])
assert LM_TRACE_DTYPE.itemsize == ctypes.sizeof(bos_lm_iteration)


class bos_plan_info(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("nnz_lower", ctypes.c_int64), ("nnz_factor", ctypes.c_int64),
                ("num_block_values", ctypes.c_int64), ("lanes_per_pose", ctypes.c_int64),
                ("flops_temporal", ctypes.c_double), ("flops_nested_dissection", ctypes.c_double),
                ("ordering", ctypes.c_char * 32), ("mf_supernodes", ctypes.c_int64),
                ("mf_levels", ctypes.c_int64), ("mf_max_front", ctypes.c_int64), ("mf_flops", ctypes.c_double),
                ("mf_update_bytes", ctypes.c_int64), ("mf_fits", ctypes.c_int64),
                ("mf_max_front_upper", ctypes.c_int64), ("mf_balance_pct", ctypes.c_int64),
                ("shard_own_fronts", ctypes.c_int64), ("shard_top_fronts", ctypes.c_int64),
                ("shard_roots", ctypes.c_int64), ("shard_ex1_doubles", ctypes.c_int64),
                ("shard_ex2_doubles", ctypes.c_int64), ("shard_pose_lanes", ctypes.c_int64),
                ("shard_own_pose_lanes", ctypes.c_int64), ("shard_lm_lanes", ctypes.c_int64),
                ("shard_update_nodes", ctypes.c_int64), ("mf_fold_fp32", ctypes.c_int64),
                ("lm_lanes_consecutive", ctypes.c_int64), ("pose_odometry_chain", ctypes.c_int64)]


_lib = None


def lib():
    """Load libbos.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BosError(f"{LIB_PATH} not built: run `make -C {_HERE}` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    sig = {
        "bos_default_options": (None, [ctypes.POINTER(bos_options)]),
        "bos_last_error": (ctypes.c_char_p, []),
        "bos_abi_version": (ctypes.c_int, []),
        "bos_device_count": (ctypes.c_int, []),
        "bos_device_peer_access": (ctypes.c_int, [ctypes.c_int32, _ip, _ip]),
        "bos_nccl_unique_id": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_create": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.POINTER(vp)]),
        "bos_destroy": (ctypes.c_int, [vp]),
        "bos_set_kernel_threshold": (ctypes.c_int, [vp, ctypes.c_double]),
        "bos_set_damping_factor": (ctypes.c_int, [vp, ctypes.c_double]),
        "bos_step": (ctypes.c_int, [vp, ctypes.POINTER(bos_step_stats)]),
        "bos_step_n": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(bos_step_stats)]),
        "bos_linearize": (ctypes.c_int, [vp, ctypes.POINTER(bos_step_stats)]),
        "bos_linearize_async": (ctypes.c_int, [vp]),
        "bos_synchronize": (ctypes.c_int, [vp]),
        "bos_triangulate": (ctypes.c_int, [vp]),
        "bos_triangulate_async": (ctypes.c_int, [vp]),
        "bos_debug_linearize_timeline": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64),
                                                        ctypes.POINTER(ctypes.c_int64), ctypes.c_int32]),
        "bos_system_info_get": (ctypes.c_int, [vp, ctypes.POINTER(bos_system_info)]),
        "bos_export_system": (ctypes.c_int, [vp, ctypes.c_int64, _ip, _ip, _dp, _dp]),
        "bos_get_state": (ctypes.c_int, [vp, _dp, _dp]),
        "bos_set_state": (ctypes.c_int, [vp, _dp, _dp]),
        "bos_get_last_dx": (ctypes.c_int, [vp, _dp]),
        "bos_dataset_load_g2o": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]),
        "bos_dataset_synthetic": (ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64,
                                                 ctypes.POINTER(vp)]),
        "bos_dataset_problem": (ctypes.c_int, [vp, ctypes.POINTER(bos_problem)]),
        "bos_dataset_pose_ids": (_ip, [vp]),
        "bos_dataset_landmark_ids": (_ip, [vp]),
        "bos_dataset_fixed_pose_id": (ctypes.c_int32, [vp]),
        "bos_dataset_bound": (ctypes.c_float, [vp]),
        "bos_dataset_ground_truth": (ctypes.c_int, [vp, ctypes.POINTER(_dp), ctypes.POINTER(_dp)]),
        "bos_dataset_write_g2o": (ctypes.c_int, [vp, ctypes.c_char_p, _dp, _dp, ctypes.c_int]),
        "bos_dataset_free": (None, [vp]),
        "bos_plan_inspect": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int32,
                                            ctypes.c_int32, ctypes.c_int64, _ip, _ip, ctypes.POINTER(ctypes.c_uint8),
                                            ctypes.POINTER(ctypes.c_uint8), _ip, ctypes.POINTER(bos_plan_info)]),
        "bos_plan_mf_selftest": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, _dp, _dp]),
        "bos_plan_mf_marginals": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, _dp, _dp]),
        "bos_marginals": (ctypes.c_int, [vp, _dp, _dp, _ip]),
        "bos_edge_covariances": (ctypes.c_int, [vp, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
        "bos_plan_mf_edge_covariances": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, _dp, _dp,
                                                         _dp, _dp, _dp, _dp]),
        "bos_edge_covariances_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_edge_consistency": (ctypes.c_int, [vp, ctypes.c_double, ctypes.c_double, ctypes.c_int32, *_EDGE_CHECK_SIG, _ip]),
        "bos_plan_mf_edge_consistency": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, ctypes.c_double,
                                                         ctypes.c_double, ctypes.c_int32, *_EDGE_CHECK_SIG]),
        "bos_edge_consistency_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_marginals_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_pair_covariances": (ctypes.c_int, [vp, ctypes.c_int64, _ip, _ip, _dp, _dp, _dp, _dp, _ip]),
        "bos_plan_mf_pair_covariances": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp,
                                                         ctypes.c_int64, _ip, _ip, _dp, _dp, _dp, _dp]),
        "bos_plan_pair_paths": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int64,
                                                _ip, _ip, _ip]),
        "bos_pair_covariances_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_debug_set_pair_batch": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_node_covariances": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
        "bos_plan_mf_node_covariances": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp,
                                                         ctypes.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, _dp]),
        "bos_node_covariances_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_associate_bearings": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_double, ctypes.c_int32, _ip, _dp, _dp,
                                                   _dp, _ip, _dp, _ip]),
        "bos_plan_mf_associate_bearings": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp,
                                                           ctypes.c_int32, _ip, _dp, _dp, ctypes.c_double, ctypes.c_int32, _ip,
                                                           _dp, _dp, _dp, _ip, _dp]),
        "bos_associate_bearings_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_debug_set_associate_chunk": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_associate_tile": (ctypes.c_int32, []),
        "bos_match_landmarks": (ctypes.c_int, [vp, ctypes.c_int32, _ip, ctypes.c_double, ctypes.c_int32, _ip, _dp, _dp, _dp, _ip, _dp,
                                               _ip]),
        "bos_match_poses": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_double, ctypes.c_int32, _ip, _dp, _dp, _dp, _ip,
                                           _dp, _ip]),
        "bos_plan_mf_match_landmarks": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, ctypes.c_int32,
                                                       _ip, ctypes.c_double, ctypes.c_int32, _ip, _dp, _dp, _dp, _ip, _dp]),
        "bos_plan_mf_match_poses": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, ctypes.c_int32, _ip,
                                                   _dp, _dp, ctypes.c_double, ctypes.c_int32, _ip, _dp, _dp, _dp, _ip, _dp]),
        "bos_match_information_inverse": (ctypes.c_int, [_dp, _dp]),
        "bos_match_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_debug_set_match_chunk": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_joint_compatibility": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _ip]),
        "bos_plan_mf_joint_compatibility": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, ctypes.c_int32,
                                                           _ip, _ip, _ip, _dp, _dp, ctypes.c_int64, _dp, _dp, _dp, _dp]),
        "bos_joint_compatibility_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_debug_set_joint_batch": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_jcbb": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _ip, _dp, _dp, _ip, _ip, _dp, ctypes.c_int64, _ip, _ip, _dp, _dp, _ip, _dp,
                                    _dp, _ip]),
        "bos_jcbb_search_host": (ctypes.c_int, [ctypes.c_int32, _ip, _ip, _dp, _dp, _dp, ctypes.c_int64, ctypes.c_int32, _ip, _ip, _dp,
                                                _dp, _ip, ctypes.POINTER(ctypes.c_int64)]),
        "bos_plan_mf_jcbb": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), _dp, ctypes.c_int32, _ip, _ip, _dp,
                                            _dp, _ip, _ip, _dp, ctypes.c_int64, ctypes.c_int64, _ip, _ip, _dp, _dp, _ip, _dp, _dp,
                                            ctypes.POINTER(ctypes.c_int64)]),
        "bos_jcbb_timing": (ctypes.c_int, [vp, _dp, ctypes.POINTER(ctypes.c_int64), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64),
                                           _ip]),
        "bos_debug_set_jcbb_batch": (ctypes.c_int, [vp, ctypes.c_int64]),
        "bos_lm_default_options": (None, [ctypes.POINTER(bos_lm_options)]),
        "bos_cost": (ctypes.c_int, [vp, _dp, _dp, _ip]),
        "bos_optimize": (ctypes.c_int, [vp, ctypes.POINTER(bos_lm_options), ctypes.POINTER(bos_lm_result),
                                        ctypes.POINTER(bos_lm_iteration), ctypes.c_int32]),
        "bos_time_cost": (ctypes.c_int, [vp, ctypes.c_int32, _dp]),
        "bos_set_priors": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_int32, _ip, _dp, _dp]),
        "bos_cpu_gn_set_priors": (ctypes.c_int, [vp, ctypes.c_int32, _ip, _dp, _dp, ctypes.c_int32, _ip, _dp, _dp]),
        "bos_prior_terms": (ctypes.c_int, [ctypes.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]),
        "bos_cpu_gn_set_kernel_threshold": (ctypes.c_int, [vp, ctypes.c_double]),
        "bos_cpu_gn_cost": (ctypes.c_int, [vp, _dp, _dp, _ip]),
        "bos_cpu_gn_optimize": (ctypes.c_int, [vp, ctypes.POINTER(bos_lm_options), ctypes.POINTER(bos_lm_result),
                                               ctypes.POINTER(bos_lm_iteration), ctypes.c_int32]),
        "bos_lm_rule_apply": (ctypes.c_int, [ctypes.POINTER(bos_lm_state), ctypes.POINTER(bos_lm_options), ctypes.c_double,
                                             ctypes.c_double, ctypes.c_double, ctypes.c_int32,
                                             ctypes.POINTER(bos_lm_iteration)]),
        "bos_plan_shard_selftest": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int32,
                                                   _dp, _dp, _dp]),
        "bos_plan_node_owner": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int32, _ip]),
        "bos_step_phase": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.POINTER(bos_step_stats)]),
        "bos_exchange_size": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
        "bos_exchange_download": (ctypes.c_int, [vp, ctypes.c_int32, _dp]),
        "bos_exchange_upload": (ctypes.c_int, [vp, ctypes.c_int32, _dp]),
        "bos_node_owner": (ctypes.c_int, [vp, _ip]),
        "bos_debug_set_g2o_parser": (None, [ctypes.c_int32]),
        "bos_debug_inject_stall": (ctypes.c_int, [vp]),
        "bos_debug_set_step_graph": (ctypes.c_int, [vp, ctypes.c_int32]),
        "bos_debug_solver_routes": (ctypes.c_int, [vp, ctypes.c_int64, _ip, _ip]),
        "bos_debug_selinv_fronts": (ctypes.c_int, [vp, ctypes.c_int64, _ip, _ip, _ip, _ip]),
        "bos_plan_mf_fronts": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int64, _ip, _ip]),
        "bos_debug_solver_stamps": (ctypes.c_int, [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64),
                                                   ctypes.POINTER(ctypes.c_int32)]),
        "bos_time_linearize": (ctypes.c_int, [vp, ctypes.c_int32, ctypes.c_int32, _dp]),
        "bos_time_triangulate": (ctypes.c_int, [vp, ctypes.c_int32, _dp]),
        "bos_time_steps": (ctypes.c_int, [vp, ctypes.c_int32, _dp]),
        "bos_cpu_gn_create": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.c_int32, ctypes.c_int32,
                                             ctypes.POINTER(vp)]),
        "bos_cpu_gn_step": (ctypes.c_int, [vp, _dp]),
        "bos_cpu_gn_get_state": (ctypes.c_int, [vp, _dp, _dp]),
        "bos_cpu_gn_destroy": (None, [vp]),
        "bos_exchange_p2p_handle": (ctypes.c_int, [vp, ctypes.c_void_p]),
        "bos_exchange_p2p_connect": (ctypes.c_int, [vp, ctypes.c_void_p]),
        "bos_set_exchange_timeout": (ctypes.c_int, [vp, ctypes.c_double]),
        "bos_last_step_stamps": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_uint64)]),
        "bos_normalized_angle_f64": (ctypes.c_double, [ctypes.c_double]),
        "bos_normalized_angle_f32": (ctypes.c_float, [ctypes.c_float]),
        "bos_time_facade_steps": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options), ctypes.c_int32,
                                                 _dp, _dp, _dp, ctypes.POINTER(ctypes.c_int64)]),
        "bos_debug_facade_selftest": (ctypes.c_int, [ctypes.POINTER(bos_problem), ctypes.POINTER(bos_options),
                                                     ctypes.c_int32, ctypes.POINTER(ctypes.c_int64)]),
    }
    for name, (res, args) in sig.items():
        if ALLOW_MISSING_SYMBOLS and not hasattr(L, name):   # A/B tools loading an older build
            continue
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != BOS_OK:
        raise BosError(f"{what} failed ({rc}): {lib().bos_last_error().decode()}")


def _ptr(a, ct):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))


def device_count() -> int:
    return lib().bos_device_count()


def device_peer_access(capacity: int = 64) -> list:
    """Peer-access matrix of the visible devices (hipDeviceCanAccessPeer; 1 on the diagonal)."""
    out = np.zeros(capacity * capacity, dtype=np.int32)
    n = np.zeros(1, dtype=np.int32)
    _check(lib().bos_device_peer_access(capacity, _ptr(out, ctypes.c_int32), _ptr(n, ctypes.c_int32)),
           "bos_device_peer_access")
    k = int(n[0])
    return out[:k * k].reshape(k, k).tolist()


class Problem:
    """SoA problem in stix order (include/bos.h bos_problem). Owns its numpy arrays."""

    def __init__(self, pose_xyt, lm_xy, b_pose, b_lm, b_z, o_src, o_dst, o_z, o_omega, fixed, b_omega=None,
                 pose_ids=None, lm_ids=None):
        self.pose_xyt = np.ascontiguousarray(pose_xyt, dtype=np.float64).reshape(-1, 3)
        self.lm_xy = np.ascontiguousarray(lm_xy, dtype=np.float64).reshape(-1, 2)
        self.b_pose = np.ascontiguousarray(b_pose, dtype=np.int32)
        self.b_lm = np.ascontiguousarray(b_lm, dtype=np.int32)
        self.b_z = np.ascontiguousarray(b_z, dtype=np.float64)
        self.b_omega = None if b_omega is None else np.ascontiguousarray(b_omega, dtype=np.float64)
        self.o_src = np.ascontiguousarray(o_src, dtype=np.int32)
        self.o_dst = np.ascontiguousarray(o_dst, dtype=np.int32)
        self.o_z = np.ascontiguousarray(o_z, dtype=np.float64).reshape(-1, 3)
        self.o_omega = np.ascontiguousarray(o_omega, dtype=np.float64).reshape(-1, 3, 3)
        self.fixed = int(fixed)
        self.pose_ids = pose_ids
        self.lm_ids = lm_ids

    @property
    def NP(self):
        return len(self.pose_xyt)

    @property
    def NL(self):
        return len(self.lm_xy)

    @property
    def N(self):
        return 3 * self.NP + 2 * self.NL

    def c_struct(self) -> bos_problem:
        p = bos_problem()
        p.num_poses, p.num_landmarks = self.NP, self.NL
        p.num_bearings, p.num_odometry = len(self.b_z), len(self.o_z)
        p.pose_xyt = _ptr(self.pose_xyt, ctypes.c_double)
        p.landmark_xy = _ptr(self.lm_xy, ctypes.c_double) if self.NL else None
        p.bearing_pose = _ptr(self.b_pose, ctypes.c_int32)
        p.bearing_landmark = _ptr(self.b_lm, ctypes.c_int32)
        p.bearing_z = _ptr(self.b_z, ctypes.c_double)
        p.bearing_omega = _ptr(self.b_omega, ctypes.c_double)
        p.odom_src = _ptr(self.o_src, ctypes.c_int32)
        p.odom_dst = _ptr(self.o_dst, ctypes.c_int32)
        p.odom_z = _ptr(self.o_z, ctypes.c_double)
        p.odom_omega = _ptr(self.o_omega, ctypes.c_double)
        p.fixed_pose = self.fixed
        return p


def _problem_from_dataset(h) -> Problem:
    L = lib()
    v = bos_problem()
    _check(L.bos_dataset_problem(h, ctypes.byref(v)), "bos_dataset_problem")
    NP, NL, Mb, Mo = v.num_poses, v.num_landmarks, v.num_bearings, v.num_odometry

    def arr(p, n, dt):
        if n == 0 or not p:
            return np.zeros(0, dtype=dt)
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)

    pose_ids = arr(L.bos_dataset_pose_ids(h), NP, np.int32)
    lm_ids = arr(L.bos_dataset_landmark_ids(h), NL, np.int32)
    return Problem(arr(v.pose_xyt, 3 * NP, np.float64), arr(v.landmark_xy, 2 * NL, np.float64),
                   arr(v.bearing_pose, Mb, np.int32), arr(v.bearing_landmark, Mb, np.int32),
                   arr(v.bearing_z, Mb, np.float64), arr(v.odom_src, Mo, np.int32), arr(v.odom_dst, Mo, np.int32),
                   arr(v.odom_z, 3 * Mo, np.float64), arr(v.odom_omega, 9 * Mo, np.float64), v.fixed_pose,
                   pose_ids=pose_ids, lm_ids=lm_ids)


def load_g2o(path: str, triangulate: bool = True, verbose: bool = False) -> Problem:
    """parse_g2o + default FIX + triangulate_landmarks, in libbos.so's C++ host code."""
    L = lib()
    h = ctypes.c_void_p()
    _check(L.bos_dataset_load_g2o(path.encode(), int(triangulate), int(verbose), ctypes.byref(h)), "load_g2o")
    try:
        P = _problem_from_dataset(h)
        P.fixed_pose_id = L.bos_dataset_fixed_pose_id(h)
        P.bound = L.bos_dataset_bound(h)
    finally:
        L.bos_dataset_free(h)
    return P


def synthetic(num_poses: int, num_landmarks: int, bearings_per_pose: int, seed: int = 0xB05EED01) -> Problem:
    """Deterministic synthetic world; P.gt_pose_xyt / P.gt_lm_xy hold ground truth."""
    L = lib()
    h = ctypes.c_void_p()
    _check(L.bos_dataset_synthetic(num_poses, num_landmarks, bearings_per_pose, seed, ctypes.byref(h)), "synthetic")
    try:
        P = _problem_from_dataset(h)
        gp, gl = _dp(), _dp()
        _check(L.bos_dataset_ground_truth(h, ctypes.byref(gp), ctypes.byref(gl)), "ground_truth")
        P.gt_pose_xyt = np.ctypeslib.as_array(gp, shape=(3 * P.NP,)).reshape(-1, 3).copy()
        P.gt_lm_xy = np.ctypeslib.as_array(gl, shape=(2 * P.NL,)).reshape(-1, 2).copy()
        P.fixed_pose_id = L.bos_dataset_fixed_pose_id(h)
    finally:
        L.bos_dataset_free(h)
    return P


def write_g2o(P: Problem, path: str, pose_xyt=None, lm_xy=None, with_landmarks=True, source: Optional[str] = None):
    """Write a problem (and optionally a state) as g2o via the C++ writer."""
    L = lib()
    h = ctypes.c_void_p()
    if source is None:
        raise BosError("write_g2o needs the source g2o path (or use bearing_only_slam --dump)")
    _check(L.bos_dataset_load_g2o(source.encode(), 1, 0, ctypes.byref(h)), "load_g2o")
    try:
        pp = None if pose_xyt is None else np.ascontiguousarray(pose_xyt, dtype=np.float64)
        ll = None if lm_xy is None else np.ascontiguousarray(lm_xy, dtype=np.float64)
        _check(L.bos_dataset_write_g2o(h, path.encode(), _ptr(pp, ctypes.c_double), _ptr(ll, ctypes.c_double),
                                       int(with_landmarks)), "write_g2o")
    finally:
        L.bos_dataset_free(h)


def time_facade_steps(P: Problem, n: int, opts=None) -> dict:
    """n x proj02::Solver::step() through the C++ façade, then one read of solver.state
    (bos_time_facade_steps; the reference's loop, executables/bearing_only_slam.cpp:93-99)."""
    ms, rd, capi, bad = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    pb = P.c_struct()
    _check(lib().bos_time_facade_steps(ctypes.byref(pb), None if opts is None else ctypes.byref(opts), n,
                                       ctypes.byref(ms), ctypes.byref(rd), ctypes.byref(capi), ctypes.byref(bad)),
           "bos_time_facade_steps")
    return {"ms_per_step": ms.value, "ms_state_read": rd.value, "ms_per_step_capi": capi.value,
            "state_mismatches": bad.value}


def facade_selftest(P: Problem, n: int, opts=None) -> int:
    """Doubles of the façade's solver.state that differ from the device state (bos_debug_facade_selftest)."""
    bad = ctypes.c_int64()
    pb = P.c_struct()
    _check(lib().bos_debug_facade_selftest(ctypes.byref(pb), None if opts is None else ctypes.byref(opts), n,
                                           ctypes.byref(bad)), "bos_debug_facade_selftest")
    return bad.value


def options(solver: int = BOS_SOLVER_SUPERNODAL, partition: int = BOS_PARTITION_SUBTREE, lanes_per_pose: int = 0,
            schur_leaf: int = 0, precision: int = BOS_FP64) -> bos_options:
    """bos_options with the planning fields set (bos_default_options for the rest)."""
    o = bos_options()
    lib().bos_default_options(ctypes.byref(o))
    o.solver, o.partition, o.lanes_per_pose, o.schur_leaf, o.precision = solver, partition, lanes_per_pose, schur_leaf, precision
    return o


def plan_inspect(P: Problem, rank: int = 0, world: int = 1, entries: bool = False,
                 solver: int = BOS_SOLVER_SUPERNODAL, partition: int = BOS_PARTITION_SUBTREE, lanes_per_pose: int = 0,
                 schur_leaf: int = 0):
    """Host-only plan build (ordering, CSR layout, shard ownership) — no GPU needed."""
    L = lib()
    cs = P.c_struct()
    info = bos_plan_info()
    opt = options(solver, partition, lanes_per_pose, schur_leaf)
    _check(L.bos_plan_inspect(ctypes.byref(cs), ctypes.byref(opt), rank, world, 0, None, None, None, None, None,
                              ctypes.byref(info)), "plan_inspect")
    out = {"n": info.n, "nnz_lower": info.nnz_lower, "nnz_factor": info.nnz_factor,
           "num_block_values": info.num_block_values, "lanes_per_pose": info.lanes_per_pose,
           "flops_temporal": info.flops_temporal, "flops_nested_dissection": info.flops_nested_dissection,
           "ordering": info.ordering.decode(), "mf_supernodes": info.mf_supernodes,
           "mf_levels": info.mf_levels, "mf_max_front": info.mf_max_front, "mf_flops": info.mf_flops,
           "mf_update_bytes": info.mf_update_bytes, "mf_fits": bool(info.mf_fits),
           "mf_max_front_upper": info.mf_max_front_upper, "mf_balance_pct": info.mf_balance_pct,
           "mf_fold_fp32": bool(info.mf_fold_fp32), "lm_lanes_consecutive": info.lm_lanes_consecutive,
           "pose_odometry_chain": info.pose_odometry_chain}
    out.update({k: getattr(info, k) for k, _ in bos_plan_info._fields_ if k.startswith("shard_")})
    if entries:
        nnz = info.nnz_lower
        rows = np.zeros(nnz, dtype=np.int32)
        cols = np.zeros(nnz, dtype=np.int32)
        owned = np.zeros(nnz, dtype=np.uint8)
        b_owned = np.zeros(P.N, dtype=np.uint8)
        perm = np.zeros(P.N, dtype=np.int32)
        _check(L.bos_plan_inspect(ctypes.byref(cs), ctypes.byref(opt), rank, world, nnz, _ptr(rows, ctypes.c_int32),
                                  _ptr(cols, ctypes.c_int32), _ptr(owned, ctypes.c_uint8),
                                  _ptr(b_owned, ctypes.c_uint8), _ptr(perm, ctypes.c_int32), None), "plan_inspect")
        out.update(rows=rows, cols=cols, owned=owned.astype(bool), b_owned=b_owned.astype(bool), perm_to_ref=perm)
    return out


def plan_mf_selftest(P: Problem, vals, rhs, solver: int = BOS_SOLVER_SUPERNODAL, schur_leaf: int = 0):
    """Host re-run of the GPU multifrontal algorithm on the plan's tree (test hook)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    b = np.ascontiguousarray(rhs, dtype=np.float64)
    x = np.zeros_like(b)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_selftest(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double),
                                      _ptr(b, ctypes.c_double), _ptr(x, ctypes.c_double)), "plan_mf_selftest")
    return x


def plan_mf_marginals(P: Problem, vals, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0):
    """Host selected inverse of the plan's multifrontal factor (test hook): the marginal covariance
    blocks (pose_cov [NP, 3, 3], lm_cov [NL, 2, 2]) of the H_nf whose stored entries are vals."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    pose = np.zeros((P.NP, 3, 3))
    lm = np.zeros((P.NL, 2, 2))
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_marginals(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double),
                                       _ptr(pose, ctypes.c_double), _ptr(lm, ctypes.c_double)), "plan_mf_marginals")
    return pose, lm


def _edge_cov_arrays(P: Problem, cross: bool, projected: bool, blocks: bool) -> dict:
    """The output arrays of an edge-covariance call; None where not asked for."""
    Mb, Mo = len(P.b_z), len(P.o_z)
    return {"bearing_cross": np.zeros((Mb, 3, 2)) if cross else None,
            "odom_cross": np.zeros((Mo, 3, 3)) if cross else None,
            "bearing_var": np.zeros(Mb) if projected else None,
            "odom_cov": np.zeros((Mo, 3, 3)) if projected else None,
            "pose_cov": np.zeros((P.NP, 3, 3)) if blocks else None,
            "landmark_cov": np.zeros((P.NL, 2, 2)) if blocks else None}


_EDGE_COV_ORDER = ("bearing_cross", "odom_cross", "bearing_var", "odom_cov", "pose_cov", "landmark_cov")


def plan_mf_edge_covariances(P: Problem, vals, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0):
    """Host form of Solver.edge_covariances() (test hook, bos_plan_mf_edge_covariances): the host
    selected inverse of the H_nf whose stored entries are vals, the edges' cross blocks through the
    plan's cross records and the projection at P's state. Returns the dict of arrays (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    out = _edge_cov_arrays(P, True, True, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_edge_covariances(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double),
                                              *[_ptr(out[k], ctypes.c_double) for k in _EDGE_COV_ORDER]),
           "plan_mf_edge_covariances")
    return out


EDGE_CHECK_MAX_K = 8   # include/bos.h BOS_EDGE_CHECK_MAX_K
# bytes of one kind's lists as a call downloads them: sizeof(bos::dev::EdgeCheckLists), pinned by a static_assert in
# csrc/hip/edge_check.hpp
EDGE_CHECK_LIST_BYTES = 936
_EDGE_CHECK_ORDER = ("cand_bearing", "cand_bearing_w2", "cand_bearing_innovation", "cand_bearing_resvar", "n_over_bearing",
                     "cand_odom", "cand_odom_w2", "cand_odom_innovation", "cand_odom_rescov", "n_over_odom",
                     "bearing_w2", "bearing_chi2", "bearing_redundancy", "odom_w2", "odom_chi2", "odom_redundancy")


def _edge_check_arrays(P: Problem, k: int, lists: bool, rows: bool, kinds=("bearing", "odom")) -> dict:
    """The output arrays of an edge-consistency call in the C argument order; None where not asked for."""
    Mb, Mo, k = len(P.b_z), len(P.o_z), max(int(k), 0)
    b, o = "bearing" in kinds, "odom" in kinds
    shape = {"cand_bearing": (k,), "cand_bearing_w2": (k,), "cand_bearing_innovation": (k,), "cand_bearing_resvar": (k,),
             "n_over_bearing": (1,), "cand_odom": (k,), "cand_odom_w2": (k,), "cand_odom_innovation": (k, 3),
             "cand_odom_rescov": (k, 3, 3), "n_over_odom": (1,), "bearing_w2": (Mb,), "bearing_chi2": (Mb,),
             "bearing_redundancy": (Mb,), "odom_w2": (Mo,), "odom_chi2": (Mo,), "odom_redundancy": (Mo,)}
    out = {}
    for key in _EDGE_CHECK_ORDER:
        want = (b if "bearing" in key else o) and (lists if key.startswith(("cand_", "n_over_")) else rows)
        integer = key.startswith("n_over_") or key in ("cand_bearing", "cand_odom")
        out[key] = np.zeros(shape[key], dtype=np.int32 if integer else np.float64) if want else None
    return out


def _edge_check_pointers(out: dict) -> list:
    return [_ptr(out[key], ctypes.c_int32 if out[key] is not None and out[key].dtype == np.int32 else ctypes.c_double)
            for key in _EDGE_CHECK_ORDER]


def _edge_check_result(out: dict) -> dict:
    for key in ("n_over_bearing", "n_over_odom"):
        out[key] = None if out[key] is None else int(out[key][0])
    return out


def plan_mf_edge_consistency(P: Problem, vals, gate_bearing: float = 0.0, gate_odom: float = 0.0, k: int = 4, rows: bool = True,
                             solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> dict:
    """Host form of Solver.edge_consistency() (test hook, bos_plan_mf_edge_consistency): the host selected inverse
    of the H_nf whose stored entries are vals, then every edge's e, T, w2, chi2 and redundancy at P's state and a
    plain stable sort. Returns the dict of arrays (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    out = _edge_check_arrays(P, k, True, rows)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_edge_consistency(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), gate_bearing, gate_odom, k,
                                              *_edge_check_pointers(out)), "plan_mf_edge_consistency")
    return _edge_check_result(out)


_PAIR_COV_ORDER = ("cross", "projected", "cov_a", "cov_b")


def _pair_cov_arrays(node_a, node_b, cross: bool, projected: bool, blocks: bool):
    """(node_a, node_b as int32 arrays, the output dict of a pair-covariance call): [n, 9] each, None
    where not asked for."""
    a = np.ascontiguousarray(node_a, dtype=np.int32).ravel()
    b = np.ascontiguousarray(node_b, dtype=np.int32).ravel()
    if len(a) != len(b):
        raise BosError("pair covariances: node_a and node_b differ in length")
    want = {"cross": cross, "projected": projected, "cov_a": blocks, "cov_b": blocks}
    return a, b, {k: np.zeros((len(a), 9)) if want[k] else None for k in _PAIR_COV_ORDER}


def pair_block(out, key: str, q: int, rows: int, cols: int) -> np.ndarray:
    """Pair q's rows x cols block of one output of a pair-covariance call (row-major in the first
    rows * cols of its nine entries)."""
    return out[key][q, :rows * cols].reshape(rows, cols)


def plan_mf_pair_covariances(P: Problem, vals, node_a, node_b, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> dict:
    """Host form of Solver.pair_covariances() (test hook, bos_plan_mf_pair_covariances): the root-path
    solves and products over the host factorization of the H_nf whose stored entries are vals, projected
    at P's state. Returns the dict of [n, 9] arrays (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, b, out = _pair_cov_arrays(node_a, node_b, True, True, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_pair_covariances(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a),
                                              _ptr(a, ctypes.c_int32), _ptr(b, ctypes.c_int32),
                                              *[_ptr(out[k], ctypes.c_double) for k in _PAIR_COV_ORDER]),
           "plan_mf_pair_covariances")
    return out


_NODE_COV_ORDER = ("cross_pose", "cross_landmark", "projected_pose", "projected_landmark", "pose_cov", "landmark_cov")


def _node_cov_arrays(P: Problem, nodes, cross: bool, projected: bool, marginals: bool):
    """(nodes as an int32 array, the output dict of a node-covariance call): cross_pose [n, NP, 9],
    cross_landmark [n, NL, 6], projected_pose [n, NP, 9], projected_landmark [n, NL, 4], pose_cov [NP, 3, 3],
    landmark_cov [NL, 2, 2]; None where not asked for."""
    a = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
    n = len(a)
    return a, {"cross_pose": np.zeros((n, P.NP, 9)) if cross else None,
               "cross_landmark": np.zeros((n, P.NL, 6)) if cross else None,
               "projected_pose": np.zeros((n, P.NP, 9)) if projected else None,
               "projected_landmark": np.zeros((n, P.NL, 4)) if projected else None,
               "pose_cov": np.zeros((P.NP, 3, 3)) if marginals else None,
               "landmark_cov": np.zeros((P.NL, 2, 2)) if marginals else None}


def plan_mf_node_covariances(P: Problem, vals, nodes, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> dict:
    """Host form of Solver.node_covariances() (test hook, bos_plan_mf_node_covariances): per query node
    the root-path solve, the backward sweep over the host factorization of the H_nf whose stored entries
    are vals, and the gather and projection at P's state. Returns the dict of arrays, every output asked
    for (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, out = _node_cov_arrays(P, nodes, True, True, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_node_covariances(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a),
                                              _ptr(a, ctypes.c_int32), *[_ptr(out[k], ctypes.c_double) for k in _NODE_COV_ORDER]),
           "plan_mf_node_covariances")
    return out


ASSOC_MAX_K = 8   # include/bos.h BOS_ASSOC_MAX_K
_ASSOC_ORDER = ("cand_landmark", "cand_nis", "cand_innovation", "cand_var", "n_inside", "nis_all")


def _assoc_arrays(P: Problem, pose, z, omega, k: int, nis_all: bool):
    """(pose, z, omega as arrays (omega None stays None), the output dict of an association call):
    cand_landmark [n, k] int32, cand_nis / cand_innovation / cand_var [n, k], n_inside [n] int32, nis_all
    [n, NL] or None. k outside 1 .. ASSOC_MAX_K is left to the library to refuse: the arrays then get one
    column."""
    a = np.ascontiguousarray(pose, dtype=np.int32).ravel()
    zz = np.ascontiguousarray(z, dtype=np.float64).ravel()
    om = None if omega is None else np.ascontiguousarray(omega, dtype=np.float64).ravel()
    if len(zz) != len(a) or (om is not None and len(om) != len(a)):
        raise BosError("associate bearings: pose, z and omega differ in length")
    n, kk = len(a), k if 1 <= k <= ASSOC_MAX_K else 1
    return a, zz, om, {"cand_landmark": np.full((n, kk), -1, dtype=np.int32), "cand_nis": np.full((n, kk), np.inf),
                       "cand_innovation": np.zeros((n, kk)), "cand_var": np.zeros((n, kk)),
                       "n_inside": np.zeros(n, dtype=np.int32), "nis_all": np.zeros((n, P.NL)) if nis_all else None}


def _assoc_ptrs(out):
    return [_ptr(out[k], ctypes.c_int32 if out[k] is not None and out[k].dtype == np.int32 else ctypes.c_double) for k in _ASSOC_ORDER]


def plan_mf_associate_bearings(P: Problem, vals, pose, z, omega=None, gate: float = np.inf, k: int = 4,
                               solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> dict:
    """Host form of Solver.associate_bearings() (test hook, bos_plan_mf_associate_bearings): the node
    column of each distinct pose over the host factorization of the H_nf whose stored entries are vals, the
    innovations at P's state and a plain sort. Returns the dict of arrays, nis_all included (no
    solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, zz, om, out = _assoc_arrays(P, pose, z, omega, k, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_associate_bearings(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a),
                                                _ptr(a, ctypes.c_int32), _ptr(zz, ctypes.c_double), _ptr(om, ctypes.c_double),
                                                gate, k, *_assoc_ptrs(out)),
           "plan_mf_associate_bearings")
    return out


def associate_tile() -> int:
    """Landmarks per workgroup of the association's first selection stage (test constant, bos_associate_tile)."""
    return lib().bos_associate_tile()


JOINT_MAX_M = 32   # include/bos.h BOS_JOINT_MAX_M
_JOINT_ORDER = ("prefix_nis", "joint_nis", "innovation", "innovation_cov")


def _joint_arrays(hypotheses, z, omega, cov: bool):
    """(hyp_start, pose, landmark, z, omega as arrays (omega None stays None), the output dict of a joint
    compatibility call). With z None `hypotheses` is a list of (pose, landmark, z[, omega]) arrays, one tuple
    per hypothesis (omega: all of them carry one, or none does); otherwise it is (hyp_start, pose, landmark)
    and z / omega are the flat arrays. innovation_cov is flat here (_joint_finish splits it), None without
    cov. Ill-formed hyp_start is left to the library to refuse."""
    if z is None:
        hyps = [tuple(np.atleast_1d(np.asarray(x)).ravel() for x in h) for h in hypotheses]
        with_om = [len(h) > 3 for h in hyps]
        if any(with_om) and not all(with_om):
            raise BosError("joint compatibility: some hypotheses carry omega, some do not")
        if any(len(h) < 3 or len({len(x) for x in h}) != 1 for h in hyps):
            raise BosError("joint compatibility: a hypothesis's arrays differ in length")
        cat = lambda i, dt: np.ascontiguousarray(np.concatenate([h[i] for h in hyps]) if hyps else [], dtype=dt)
        start = np.zeros(len(hyps) + 1, dtype=np.int32)
        start[1:] = np.cumsum([len(h[0]) for h in hyps])
        a, l, zz = cat(0, np.int32), cat(1, np.int32), cat(2, np.float64)
        om = cat(3, np.float64) if hyps and all(with_om) else None
    else:
        start, a, l = (np.ascontiguousarray(x, dtype=np.int32).ravel() for x in hypotheses)
        zz = np.ascontiguousarray(z, dtype=np.float64).ravel()
        om = None if omega is None else np.ascontiguousarray(omega, dtype=np.float64).ravel()
        if len(start) < 1 or len(l) != len(a) or len(zz) != len(a) or (om is not None and len(om) != len(a)) or \
                (len(start) > 1 and start[-1] != len(a)):
            raise BosError("joint compatibility: the arrays do not match hyp_start")
    m = np.maximum(np.diff(start.astype(np.int64)), 0)
    out = {"prefix_nis": np.zeros(len(a)), "joint_nis": np.zeros(len(start) - 1), "innovation": np.zeros(len(a)),
           "innovation_cov": np.zeros(int(np.sum(m * m))) if cov else None}
    return start, a, l, zz, om, out


def _joint_finish(start, out):
    """innovation_cov as a list of m x m arrays (views of the flat output), and hyp_start"""
    if out["innovation_cov"] is not None:
        m = np.diff(start.astype(np.int64))
        off = np.concatenate([[0], np.cumsum(m * m)])
        flat = out["innovation_cov"]
        out["innovation_cov"] = [flat[off[h]:off[h + 1]].reshape(m[h], m[h]) for h in range(len(m))]
    out["hyp_start"] = start
    return out


def plan_mf_joint_compatibility(P: Problem, vals, hypotheses, z=None, omega=None, solver: int = BOS_SOLVER_SCHUR,
                                schur_leaf: int = 0, max_batch: int = 0) -> dict:
    """Host form of Solver.joint_compatibility() (test hook, bos_plan_mf_joint_compatibility): the pair hook's
    path solves and products over the host factorization of the H_nf whose stored entries are vals, then S,
    its LDL^T and the prefix NIS by the code the device kernel runs, at P's state. max_batch > 0 closes a
    batch at that many hypotheses. Returns the dict of arrays, innovation_cov included (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    start, a, l, zz, om, out = _joint_arrays(hypotheses, z, omega, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_joint_compatibility(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(start) - 1,
                                                 _ptr(start, ctypes.c_int32), _ptr(a, ctypes.c_int32), _ptr(l, ctypes.c_int32),
                                                 _ptr(zz, ctypes.c_double), _ptr(om, ctypes.c_double), max_batch,
                                                 *[_ptr(out[k], ctypes.c_double) for k in _JOINT_ORDER]),
           "plan_mf_joint_compatibility")
    return _joint_finish(start, out)


JCBB_MAX_BEARINGS = 32   # include/bos.h BOS_JCBB_MAX_BEARINGS


def _jcbb_lists(candidates):
    """(cand_start, cand_landmark) of one frame's candidate lists: a list of lists, or a 2-D array with -1
    padding such as associate_bearings()["cand_landmark"] (the -1 entries are dropped)."""
    lists = [np.atleast_1d(np.asarray(c, dtype=np.int64)).ravel() for c in candidates]
    lists = [c[c != -1] for c in lists]
    start = np.zeros(len(lists) + 1, dtype=np.int64)
    start[1:] = np.cumsum([len(c) for c in lists])
    return start, (np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64))


def _jcbb_arrays(frames, gate, cov: bool, detail: bool = True):
    """(the call's input arrays as a dict, the output dict) of a jcbb call. `frames` is a list of
    (pose, z, omega_or_None, candidates), one tuple per frame: pose [m] (or one stix for all), z [m], omega [m]
    or None (all frames carry one, or none does) and the candidate lists (_jcbb_lists); or a dict of the raw
    arrays frame_start, pose, z, omega (may be None), cand_start, cand_landmark, handed to the library as they
    are. Outputs not asked for are None."""
    if isinstance(frames, dict):
        a = {"frame_start": np.ascontiguousarray(frames["frame_start"], dtype=np.int32).ravel(),
             "pose": np.ascontiguousarray(frames["pose"], dtype=np.int32).ravel(),
             "z": np.ascontiguousarray(frames["z"], dtype=np.float64).ravel(),
             "omega": None if frames.get("omega") is None else np.ascontiguousarray(frames["omega"], dtype=np.float64).ravel(),
             "cand_start": np.ascontiguousarray(frames["cand_start"], dtype=np.int32).ravel(),
             "cand_landmark": np.ascontiguousarray(frames["cand_landmark"], dtype=np.int32).ravel()}
        nb, npair = len(a["pose"]), len(a["cand_landmark"])
        # the library has no lengths to check the ends against: frame_start must end at the bearings given and
        # cand_start at the candidates given (a decreasing array is left to the library, which refuses it before it
        # reads what the array indexes)
        if len(a["frame_start"]) < 1 or len(a["z"]) != nb or (a["omega"] is not None and len(a["omega"]) != nb) or \
                len(a["cand_start"]) != nb + 1 or \
                (len(a["frame_start"]) > 1 and a["frame_start"][-1] != nb and np.all(np.diff(a["frame_start"]) >= 0)) or \
                (a["cand_start"][-1] != npair and np.all(np.diff(a["cand_start"]) >= 0)):
            raise BosError("jcbb: the ends of frame_start / cand_start do not agree with the arrays")
    else:
        zs = [np.atleast_1d(np.asarray(f[1], dtype=np.float64)).ravel() for f in frames]
        poses = [np.broadcast_to(np.atleast_1d(np.asarray(f[0], dtype=np.int64)).ravel(), zs[i].shape) if np.size(f[0]) == 1
                 else np.atleast_1d(np.asarray(f[0], dtype=np.int64)).ravel() for i, f in enumerate(frames)]
        with_om = [f[2] is not None for f in frames]
        if any(with_om) and not all(with_om):
            raise BosError("jcbb: some frames carry omega, some do not")
        oms = [np.atleast_1d(np.asarray(f[2], dtype=np.float64)).ravel() for f in frames] if frames and all(with_om) else None
        lists = [_jcbb_lists(f[3]) for f in frames]
        for i in range(len(frames)):
            if len(poses[i]) != len(zs[i]) or len(lists[i][0]) != len(zs[i]) + 1 or (oms is not None and len(oms[i]) != len(zs[i])):
                raise BosError("jcbb: a frame's arrays differ in length")
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs) if xs else [], dtype=dt)
        frame_start = np.zeros(len(frames) + 1, dtype=np.int32)
        frame_start[1:] = np.cumsum([len(x) for x in zs])
        cand_start = np.zeros(int(frame_start[-1]) + 1, dtype=np.int64)
        off = 0
        for i, (st, _) in enumerate(lists):
            cand_start[frame_start[i]:frame_start[i + 1] + 1] = st + off
            off += st[-1]
        a = {"frame_start": frame_start, "pose": cat(poses, np.int32), "z": cat(zs, np.float64),
             "omega": None if oms is None else cat(oms, np.float64), "cand_start": cand_start.astype(np.int32),
             "cand_landmark": cat([l for _, l in lists], np.int32)}
        nb, npair = len(a["pose"]), len(a["cand_landmark"])
    a["gate"] = np.ascontiguousarray(gate, dtype=np.float64).ravel()
    if len(a["gate"]) != JOINT_MAX_M:
        raise BosError(f"jcbb: gate needs {JOINT_MAX_M} entries")
    nf = len(a["frame_start"]) - 1
    fs, cs = a["frame_start"].astype(np.int64), a["cand_start"].astype(np.int64)
    ok = len(fs) > 0 and np.all(fs >= 0) and np.all(fs <= nb)
    pf = np.maximum(np.diff(cs[fs]), 0) if ok else np.zeros(nf, dtype=np.int64)
    out = {"assignment": np.full(nb, -1, dtype=np.int32),
           "n_paired": np.zeros(nf, dtype=np.int32) if detail else None,
           "joint_nis": np.zeros(nf) if detail else None,
           "prefix_nis": np.zeros(nb) if detail else None,
           "complete": np.zeros(nf, dtype=np.int32) if detail else None,
           "innovation": np.zeros(npair) if detail else None,
           "innovation_cov": np.zeros(int(np.sum(pf * pf))) if cov else None}
    return a, out


def _jcbb_out_ptrs(out):
    return [_ptr(out["assignment"], ctypes.c_int32), _ptr(out["n_paired"], ctypes.c_int32), _ptr(out["joint_nis"], ctypes.c_double),
            _ptr(out["prefix_nis"], ctypes.c_double), _ptr(out["complete"], ctypes.c_int32), _ptr(out["innovation"], ctypes.c_double),
            _ptr(out["innovation_cov"], ctypes.c_double)]


def _jcbb_finish(a, out):
    """innovation_cov as a list of P x P arrays (views of the flat output); the lists the call was given"""
    if out["innovation_cov"] is not None:
        pf = np.diff(a["cand_start"].astype(np.int64)[a["frame_start"]])
        off = np.concatenate([[0], np.cumsum(pf * pf)])
        flat = out["innovation_cov"]
        out["innovation_cov"] = [flat[off[f]:off[f + 1]].reshape(pf[f], pf[f]) for f in range(len(pf))]
    for k in ("frame_start", "cand_start", "cand_landmark"):
        out[k] = a[k]
    return out


def jcbb_search_host(candidates, S, e, gate, max_nodes: int = 0, no_bound: bool = False) -> dict:
    """The serial search of Solver.jcbb() on a given all-pairings system (test hook, bos_jcbb_search_host): one
    frame with the candidate lists `candidates` (_jcbb_lists), S [P, P], e [P], gate [JOINT_MAX_M]. no_bound
    switches the count and NIS bound off. Returns a dict with assignment [m], n_paired, joint_nis, prefix_nis
    [m], complete and nodes (the nodes visited)."""
    start, lm = _jcbb_lists(candidates)
    m = len(start) - 1
    start, lm = np.ascontiguousarray(start, dtype=np.int32), np.ascontiguousarray(lm, dtype=np.int32)
    S = np.ascontiguousarray(S, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64).ravel()
    g = np.ascontiguousarray(gate, dtype=np.float64).ravel()
    if S.size != len(lm) * len(lm) or len(e) != len(lm) or len(g) != JOINT_MAX_M:
        raise BosError("jcbb_search_host: S, e or gate do not match the lists")
    assignment, prefix = np.full(m, -1, dtype=np.int32), np.zeros(m)
    n, c, nis, nodes = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0.0), ctypes.c_int64(0)
    _check(lib().bos_jcbb_search_host(m, _ptr(start, ctypes.c_int32), _ptr(lm, ctypes.c_int32), _ptr(S, ctypes.c_double),
                                      _ptr(e, ctypes.c_double), _ptr(g, ctypes.c_double), max_nodes, 1 if no_bound else 0,
                                      _ptr(assignment, ctypes.c_int32), ctypes.byref(n), ctypes.byref(nis),
                                      _ptr(prefix, ctypes.c_double), ctypes.byref(c), ctypes.byref(nodes)),
           "jcbb_search_host")
    return {"assignment": assignment, "n_paired": n.value, "joint_nis": nis.value, "prefix_nis": prefix, "complete": c.value,
            "nodes": nodes.value}


def plan_mf_jcbb(P: Problem, vals, frames, gate, max_nodes: int = 0, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0,
                 max_batch: int = 0) -> dict:
    """Host form of Solver.jcbb() (test hook, bos_plan_mf_jcbb): the frames' all-pairings hypotheses through
    plan_mf_joint_compatibility's code over the host factorization of the H_nf whose stored entries are vals,
    then the serial search per frame, at P's state. max_batch > 0 closes a batch at that many frames. Returns
    the dict of Solver.jcbb(), innovation_cov included, with nodes [n_frames] and without solver_info."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, out = _jcbb_arrays(frames, gate, True)
    nodes = np.zeros(len(a["frame_start"]) - 1, dtype=np.int64)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_jcbb(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a["frame_start"]) - 1,
                                  _ptr(a["frame_start"], ctypes.c_int32), _ptr(a["pose"], ctypes.c_int32),
                                  _ptr(a["z"], ctypes.c_double), _ptr(a["omega"], ctypes.c_double),
                                  _ptr(a["cand_start"], ctypes.c_int32), _ptr(a["cand_landmark"], ctypes.c_int32),
                                  _ptr(a["gate"], ctypes.c_double), max_nodes, max_batch, *_jcbb_out_ptrs(out),
                                  _ptr(nodes, ctypes.c_int64)),
           "plan_mf_jcbb")
    out["nodes"] = nodes
    return _jcbb_finish(a, out)


MATCH_MAX_K = ASSOC_MAX_K   # include/bos.h BOS_MATCH_MAX_K
_MATCH_LM_ORDER = ("cand_landmark", "cand_d2", "cand_diff", "cand_cov", "n_inside", "d2_all")
_MATCH_POSE_ORDER = ("cand_pose", "cand_nis", "cand_innovation", "cand_cov", "n_inside", "nis_all")


def _match_outputs(order, n: int, k: int, N: int, dd: int, dc: int, want_all: bool) -> dict:
    """The output dict of a matching call in the order of its C arguments: indices [n, k] int32, scores
    [n, k], details [n, k, dd], covariances [n, k, dc], n_inside [n] int32, the rows [n, N] or None. k
    outside 1 .. MATCH_MAX_K is left to the library to refuse: the arrays then get one column."""
    kk = k if 1 <= k <= MATCH_MAX_K else 1
    return {order[0]: np.full((n, kk), -1, dtype=np.int32), order[1]: np.full((n, kk), np.inf),
            order[2]: np.zeros((n, kk, dd)), order[3]: np.zeros((n, kk, dc)), order[4]: np.zeros(n, dtype=np.int32),
            order[5]: np.zeros((n, N)) if want_all else None}


def _match_lm_arrays(P: Problem, landmarks, k: int, d2_all: bool):
    a = np.ascontiguousarray(landmarks, dtype=np.int32).ravel()
    return a, _match_outputs(_MATCH_LM_ORDER, len(a), k, P.NL, 2, 4, d2_all)


def _match_pose_arrays(P: Problem, pose, z, omega, k: int, nis_all: bool):
    """(pose [n], z [n, 3], omega [n, 9] or None, the output dict): one omega (3 x 3) serves every
    measurement."""
    a = np.ascontiguousarray(pose, dtype=np.int32).ravel()
    zz = np.ascontiguousarray(z, dtype=np.float64).reshape(-1, 3)
    om = None
    if omega is not None:
        om = np.asarray(omega, dtype=np.float64)
        om = np.ascontiguousarray(np.broadcast_to(om.reshape(1, 9), (len(a), 9)) if om.size == 9 else om.reshape(-1, 9))
    if len(zz) != len(a) or (om is not None and len(om) != len(a)):
        raise BosError("match poses: pose, z and omega differ in length")
    return a, zz, om, _match_outputs(_MATCH_POSE_ORDER, len(a), k, P.NP, 3, 9, nis_all)


def _match_ptrs(out, order):
    return [_ptr(out[k], ctypes.c_int32 if out[k] is not None and out[k].dtype == np.int32 else ctypes.c_double) for k in order]


def plan_mf_match_landmarks(P: Problem, vals, landmarks, gate: float = np.inf, k: int = 4, solver: int = BOS_SOLVER_SCHUR,
                            schur_leaf: int = 0) -> dict:
    """Host form of Solver.match_landmarks() (test hook, bos_plan_mf_match_landmarks): the node column of
    each query landmark over the host factorization of the H_nf whose stored entries are vals, the
    distances at P's state and a plain sort. Returns the dict of arrays, d2_all included (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, out = _match_lm_arrays(P, landmarks, k, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_match_landmarks(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a),
                                             _ptr(a, ctypes.c_int32), gate, k, *_match_ptrs(out, _MATCH_LM_ORDER)),
           "plan_mf_match_landmarks")
    return out


def plan_mf_match_poses(P: Problem, vals, pose, z, omega=None, gate: float = np.inf, k: int = 4, solver: int = BOS_SOLVER_SCHUR,
                        schur_leaf: int = 0) -> dict:
    """Host form of Solver.match_poses() (test hook, bos_plan_mf_match_poses). Returns the dict of arrays,
    nis_all included (no solver_info)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    a, zz, om, out = _match_pose_arrays(P, pose, z, omega, k, True)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_mf_match_poses(ctypes.byref(cs), ctypes.byref(opt), _ptr(v, ctypes.c_double), len(a),
                                         _ptr(a, ctypes.c_int32), _ptr(zz, ctypes.c_double), _ptr(om, ctypes.c_double), gate, k,
                                         *_match_ptrs(out, _MATCH_POSE_ORDER)),
           "plan_mf_match_poses")
    return out


def match_information_inverse(omega) -> np.ndarray:
    """R = omega^-1 (3 x 3) with the bits Solver.match_poses() uses (bos_match_information_inverse)."""
    om = np.ascontiguousarray(omega, dtype=np.float64).reshape(9)
    R = np.zeros(9)
    _check(lib().bos_match_information_inverse(_ptr(om, ctypes.c_double), _ptr(R, ctypes.c_double)), "bos_match_information_inverse")
    return R.reshape(3, 3)


# columns of plan_pair_paths
PAIR_PATH_COLS = ("sn_a", "sn_b", "lca", "common_dofs", "longest_path_dofs")


def plan_pair_paths(P: Problem, node_a, node_b, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> np.ndarray:
    """The root paths of node pairs from the plan alone (bos_plan_pair_paths): [n, 5] int32 with the
    columns PAIR_PATH_COLS: supernode of a, supernode of b (-1: the fixed pose), their lowest common
    ancestor (-1: none, -2: the pair involves the fixed pose), the dofs the two paths share and the
    longer path in dofs."""
    cs = P.c_struct()
    a, b, _ = _pair_cov_arrays(node_a, node_b, False, False, False)
    out = np.zeros((len(a), len(PAIR_PATH_COLS)), dtype=np.int32)
    opt = options(solver, schur_leaf=schur_leaf)
    _check(lib().bos_plan_pair_paths(ctypes.byref(cs), ctypes.byref(opt), len(a), _ptr(a, ctypes.c_int32),
                                     _ptr(b, ctypes.c_int32), _ptr(out, ctypes.c_int32)), "plan_pair_paths")
    return out


# columns of plan_mf_fronts (bos_host.h BOS_PLAN_FRONT_COLS)
PLAN_FRONT_COLS = ("k", "r", "level", "parent", "children", "folded_children", "folded", "diag_records", "cross_rj",
                   "cross_jj", "cross_transposed")


def plan_mf_fronts(P: Problem, solver: int = BOS_SOLVER_SCHUR, schur_leaf: int = 0) -> np.ndarray:
    """The fronts of the plan's multifrontal tree, host only (bos_plan_mf_fronts): [nsuper, 11] int32
    with the columns PLAN_FRONT_COLS: k, r, tree level (-1: a folded landmark), parent (-1: a root),
    children, folded children, 1 when the supernode itself is folded, and the selected inverse's records
    of the front: whole nodes, cross records reading S_RJ, evaluating S_JJ, and the transposed ones."""
    cs = P.c_struct()
    opt = options(solver, schur_leaf=schur_leaf)
    n = ctypes.c_int32(0)
    _check(lib().bos_plan_mf_fronts(ctypes.byref(cs), ctypes.byref(opt), 0, None, ctypes.byref(n)), "plan_mf_fronts")
    out = np.zeros((n.value, len(PLAN_FRONT_COLS)), dtype=np.int32)
    _check(lib().bos_plan_mf_fronts(ctypes.byref(cs), ctypes.byref(opt), out.size, _ptr(out, ctypes.c_int32),
                                    ctypes.byref(n)), "plan_mf_fronts")
    return out


def plan_shard_selftest(P: Problem, world: int, vals, rhs, solver: int = BOS_SOLVER_SCHUR):
    """Host simulation of the sharded solve over `world` ranks, exchanges included (test hook):
    raises unless the merged solution equals the one-rank solution bit for bit and every rank's J+H
    reads only nodes its box-plus keeps current; returns x (permuted order)."""
    cs = P.c_struct()
    v = np.ascontiguousarray(vals, dtype=np.float64)
    b = np.ascontiguousarray(rhs, dtype=np.float64)
    x = np.zeros_like(b)
    opt = options(solver)
    _check(lib().bos_plan_shard_selftest(ctypes.byref(cs), ctypes.byref(opt), world, _ptr(v, ctypes.c_double),
                                         _ptr(b, ctypes.c_double), _ptr(x, ctypes.c_double)), "plan_shard_selftest")
    return x


def plan_node_owner(P: Problem, world: int, solver: int = BOS_SOLVER_SCHUR) -> np.ndarray:
    """Owner rank of every node (poses, then landmarks) of a `world`-rank shard; -1 top, -2 fixed pose."""
    cs = P.c_struct()
    o = np.zeros(P.NP + P.NL, dtype=np.int32)
    opt = options(solver)
    _check(lib().bos_plan_node_owner(ctypes.byref(cs), ctypes.byref(opt), world, _ptr(o, ctypes.c_int32)),
           "plan_node_owner")
    return o


def lm_options(**opts) -> bos_lm_options:
    """bos_lm_options: the defaults (bos_lm_default_options) with the given fields replaced."""
    o = bos_lm_options()
    lib().bos_lm_default_options(ctypes.byref(o))
    names = {k for k, _ in bos_lm_options._fields_}
    for k, v in opts.items():
        if k not in names:
            raise TypeError(f"unknown LM option {k!r}")
        setattr(o, k, v)
    return o


def lm_rule_apply(state: dict, opts: bos_lm_options, cost_trial: float, predicted: float, max_abs_dx: float,
                  solver_info: int = 0):
    """One decision of the LM step control (bos_lm_rule_apply, the code the device and the CPU twin
    run): (new state dict, record dict, counted)."""
    st = bos_lm_state()
    for k, _ in bos_lm_state._fields_:
        setattr(st, k, state.get(k, 0))
    rec = bos_lm_iteration()
    rc = lib().bos_lm_rule_apply(ctypes.byref(st), ctypes.byref(opts), cost_trial, predicted, max_abs_dx, solver_info,
                                 ctypes.byref(rec))
    if rc < 0:
        _check(rc, "bos_lm_rule_apply")
    return ({k: getattr(st, k) for k, _ in bos_lm_state._fields_},
            {k: getattr(rec, k) for k, _ in bos_lm_iteration._fields_}, bool(rc))


def _run_optimize(fn, h, what, opts) -> dict:
    o = lm_options(**opts)
    cap = max(1, min(int(o.max_iterations), LM_MAX_ITERATIONS))
    trace = np.zeros(cap, dtype=LM_TRACE_DTYPE)
    res = bos_lm_result()
    _check(fn(h, ctypes.byref(o), ctypes.byref(res), trace.ctypes.data_as(ctypes.POINTER(bos_lm_iteration)), cap), what)
    out = {k: getattr(res, k) for k, _ in bos_lm_result._fields_}
    out["trace"] = trace[:res.iterations].copy()
    return out


def _run_cost(fn, h, what) -> dict:
    F, chi = ctypes.c_double(0), ctypes.c_double(0)
    nrob = ctypes.c_int32(0)
    _check(fn(h, ctypes.byref(F), ctypes.byref(chi), ctypes.byref(nrob)), what)
    return {"cost": F.value, "chi2": chi.value, "n_robust": nrob.value}


def _prior_arrays(prior, dim: int):
    """(index, mean, omega) -> contiguous (n, int32 [n], float64 [n, dim], float64 [n, dim, dim]); None: no priors."""
    if prior is None:
        return 0, None, None, None
    index, mean, omega = prior
    idx = np.ascontiguousarray(np.asarray(index, dtype=np.int32).reshape(-1))
    n = idx.size
    if n == 0:
        return 0, None, None, None
    m = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(n, dim))
    om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).reshape(n, dim, dim))
    return n, idx, m, om


def _set_priors(fn, h, what, pose, landmark):
    npp, pi, pm, po = _prior_arrays(pose, 3)
    nl, li, lmn, lo = _prior_arrays(landmark, 2)
    _check(fn(h, npp, _ptr(pi, ctypes.c_int32), _ptr(pm, ctypes.c_double), _ptr(po, ctypes.c_double),
              nl, _ptr(li, ctypes.c_int32), _ptr(lmn, ctypes.c_double), _ptr(lo, ctypes.c_double)), what)


def prior_terms(kind: str, node_state, mean, omega):
    """The terms of one prior in fp64 (bos_prior_terms): kind "pose" (state and mean of 3, omega 3 x 3) or
    "landmark" (2, 2 x 2). Returns (A, g, rho): A the lower triangle (00, 10, 11[, 20, 21, 22]) of J^T Omega J,
    g = J^T Omega e, rho = e^T Omega e."""
    dim = {"pose": 3, "landmark": 2}[kind]
    x = np.ascontiguousarray(np.asarray(node_state, dtype=np.float64).reshape(dim))
    m = np.ascontiguousarray(np.asarray(mean, dtype=np.float64).reshape(dim))
    om = np.ascontiguousarray(np.asarray(omega, dtype=np.float64).reshape(dim, dim))
    A = np.zeros(dim * (dim + 1) // 2)
    g = np.zeros(dim)
    rho = ctypes.c_double(0)
    _check(lib().bos_prior_terms(0 if kind == "pose" else 1, _ptr(x, ctypes.c_double), _ptr(m, ctypes.c_double),
                                 _ptr(om, ctypes.c_double), _ptr(A, ctypes.c_double), _ptr(g, ctypes.c_double),
                                 ctypes.byref(rho)), "bos_prior_terms")
    return A, g, rho.value


class CpuGN:
    """The CPU baseline of bench.py (include/bos_host.h bos_cpu_gn_*): the same GN iteration on the
    host's cores with the build's own host multifrontal Cholesky. Not a fallback of Solver."""

    def __init__(self, P: Problem, threads: int, solver: int = BOS_SOLVER_SCHUR):
        self.P = P
        self._h = ctypes.c_void_p()
        cs = P.c_struct()
        _check(lib().bos_cpu_gn_create(ctypes.byref(cs), solver, threads, ctypes.byref(self._h)), "bos_cpu_gn_create")

    def step(self) -> float:
        c = ctypes.c_double(0)
        _check(lib().bos_cpu_gn_step(self._h, ctypes.byref(c)), "bos_cpu_gn_step")
        return c.value

    def set_kernel_threshold(self, kt: float):
        _check(lib().bos_cpu_gn_set_kernel_threshold(self._h, kt), "bos_cpu_gn_set_kernel_threshold")

    def set_priors(self, pose=None, landmark=None):
        """The CPU twin of Solver.set_priors (bos_cpu_gn_set_priors): same arguments, replaces the set."""
        _set_priors(lib().bos_cpu_gn_set_priors, self._h, "bos_cpu_gn_set_priors", pose, landmark)

    def cost(self) -> dict:
        """The objective at the current state (bos_cpu_gn_cost): cost, chi2, n_robust."""
        return _run_cost(lib().bos_cpu_gn_cost, self._h, "bos_cpu_gn_cost")

    def optimize(self, **opts) -> dict:
        """The CPU twin of Solver.optimize (bos_cpu_gn_optimize): same options, result and trace."""
        return _run_optimize(lib().bos_cpu_gn_optimize, self._h, "bos_cpu_gn_optimize", opts)

    def get_state(self):
        pose = np.zeros((self.P.NP, 3))
        lm = np.zeros((self.P.NL, 2))
        _check(lib().bos_cpu_gn_get_state(self._h, _ptr(pose, ctypes.c_double), _ptr(lm, ctypes.c_double)),
               "bos_cpu_gn_get_state")
        return pose, lm

    def close(self):
        if self._h:
            lib().bos_cpu_gn_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def nccl_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(lib().bos_nccl_unique_id(buf, 128), "bos_nccl_unique_id")
    return buf.raw


class Solver:
    """``proj02::Solver`` over the HIP path. ``state`` is downloaded after every ``step()``."""

    def __init__(self, P: Problem, precision: int = BOS_FP64, solver: int = BOS_SOLVER_SPARSE_CHOL,
                 device: int = -1, kernel_threshold: float = 1.0, damping: float = 0.01, stream: int = 0,
                 rank: int = 0, world_size: int = 1, nccl_id: Optional[bytes] = None, triangulate: bool = False,
                 partition: int = BOS_PARTITION_SUBTREE, lanes_per_pose: int = 0, schur_leaf: int = 0):
        """triangulate=True: ignore P.lm_xy and triangulate the landmarks on the device from the
        initial poses (bos_problem.landmark_xy = NULL). partition / lanes_per_pose / schur_leaf: the
        bos_options fields of the same names."""
        L = lib()
        self.P = P
        self.partition = partition
        opt = bos_options()
        L.bos_default_options(ctypes.byref(opt))
        opt.precision, opt.solver, opt.device = precision, solver, device
        opt.kernel_threshold, opt.damping = kernel_threshold, damping
        opt.stream = stream or None
        opt.rank, opt.world_size = rank, world_size
        opt.partition, opt.lanes_per_pose, opt.schur_leaf = partition, lanes_per_pose, schur_leaf
        self._nid = None
        if nccl_id is not None:
            self._nid = ctypes.create_string_buffer(nccl_id, len(nccl_id))
            opt.nccl_unique_id = ctypes.cast(self._nid, ctypes.c_void_p)
        self._h = ctypes.c_void_p()
        cs = P.c_struct()
        if triangulate:
            cs.landmark_xy = None
        _check(L.bos_create(ctypes.byref(cs), ctypes.byref(opt), ctypes.byref(self._h)), "bos_create")
        self.last_stats = None

    def close(self):
        if self._h:
            lib().bos_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel_threshold(self, kt: float):
        _check(lib().bos_set_kernel_threshold(self._h, kt), "set_kernel_threshold")

    def set_damping_factor(self, df: float):
        _check(lib().bos_set_damping_factor(self._h, df), "set_damping_factor")

    def set_priors(self, pose=None, landmark=None):
        """Unary prior factors (bos_set_priors): pose = (index [n], mean [n, 3], omega [n, 3, 3]), landmark =
        (index [n], mean [n, 2], omega [n, 2, 2]), either may be None. Replaces the handle's whole prior set;
        every H, b, chi2 and cost the handle computes afterwards includes the priors."""
        _set_priors(lib().bos_set_priors, self._h, "bos_set_priors", pose, landmark)

    def clear_priors(self):
        """Removes every prior (bos_set_priors with two empty sets)."""
        self.set_priors(None, None)

    def step(self) -> dict:
        st = bos_step_stats()
        _check(lib().bos_step(self._h, ctypes.byref(st)), "bos_step")
        self.last_stats = st.as_dict()
        return self.last_stats

    def step_n(self, n: int) -> dict:
        st = bos_step_stats()
        _check(lib().bos_step_n(self._h, n, ctypes.byref(st)), "bos_step_n")
        self.last_stats = st.as_dict()
        return self.last_stats

    def linearize(self) -> dict:
        st = bos_step_stats()
        _check(lib().bos_linearize(self._h, ctypes.byref(st)), "bos_linearize")
        return st.as_dict()

    def linearize_async(self):
        _check(lib().bos_linearize_async(self._h), "bos_linearize_async")

    def debug_timeline(self, flush_caches: bool = False) -> np.ndarray:
        """One J+H launch with per-wave stamps (diagnostics): rows of [block, wave, kind, t_start,
        t_loop, t_loop_end, t_end, hw_id | xcc << 32], times in 100 MHz ticks; flush_caches: the
        launch reads its inputs from HBM (1 GiB read before it)."""
        n = ctypes.c_int64(0)
        _check(lib().bos_debug_linearize_timeline(self._h, 0, None, ctypes.byref(n), 0), "timeline")
        out = np.zeros((n.value, 8), dtype=np.uint64)
        _check(lib().bos_debug_linearize_timeline(self._h, n.value, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                  ctypes.byref(n), int(flush_caches)), "timeline")
        return out

    # ---- sharded (multi-GPU) step, external exchange: see include/bos.h
    def step_phase(self, phase: int):
        """One phase of an external-exchange step; returns the step's stats from its last phase
        (2 for the subtree partition, 1 for the observations partition), else None."""
        st = bos_step_stats()
        _check(lib().bos_step_phase(self._h, phase, ctypes.byref(st)), f"bos_step_phase({phase})")
        if phase == (1 if self.partition == BOS_PARTITION_OBSERVATIONS else 2):
            self.last_stats = st.as_dict()
            return self.last_stats
        return None

    def exchange_size(self, which: int) -> int:
        n = ctypes.c_int64(0)
        _check(lib().bos_exchange_size(self._h, which, ctypes.byref(n)), "bos_exchange_size")
        return n.value

    def exchange_download(self, which: int) -> np.ndarray:
        out = np.zeros(self.exchange_size(which))
        _check(lib().bos_exchange_download(self._h, which, _ptr(out, ctypes.c_double)), "bos_exchange_download")
        return out

    def exchange_upload(self, which: int, all_ranks: np.ndarray):
        """Subtree partition: every rank's buffer concatenated in rank order (all-gather);
        observations partition: the element-wise sum over the ranks (all-reduce)."""
        a = np.ascontiguousarray(all_ranks, dtype=np.float64)
        _check(lib().bos_exchange_upload(self._h, which, _ptr(a, ctypes.c_double)), "bos_exchange_upload")

    def p2p_handle(self) -> bytes:
        """This rank's direct-exchange mailbox handle (bos_exchange_p2p_handle)."""
        buf = ctypes.create_string_buffer(P2P_HANDLE_BYTES)
        _check(lib().bos_exchange_p2p_handle(self._h, buf), "bos_exchange_p2p_handle")
        return buf.raw

    def p2p_connect(self, handles) -> None:
        """Every rank's handle in rank order (bos_exchange_p2p_connect): bos_step then exchanges
        directly between the ranks' mailboxes."""
        blob = b"".join(handles)
        buf = ctypes.create_string_buffer(blob, len(blob))
        _check(lib().bos_exchange_p2p_connect(self._h, buf), "bos_exchange_p2p_connect")

    def last_step_stamps(self) -> np.ndarray:
        """Phase stamps of the last step (bos_last_step_stamps; 100 MHz realtime ticks)."""
        st = np.zeros(8, dtype=np.uint64)
        _check(lib().bos_last_step_stamps(self._h, st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
               "bos_last_step_stamps")
        return st

    def set_exchange_timeout(self, seconds: float) -> None:
        """Bound of the direct exchange's device-side flag waits (bos_set_exchange_timeout, 2 s default)."""
        _check(lib().bos_set_exchange_timeout(self._h, float(seconds)), "bos_set_exchange_timeout")

    def node_owner(self) -> np.ndarray:
        o = np.zeros(self.P.NP + self.P.NL, dtype=np.int32)
        _check(lib().bos_node_owner(self._h, _ptr(o, ctypes.c_int32)), "bos_node_owner")
        return o

    def debug_inject_stall(self):
        """Test hook: the next step's factor dataflow launch skips its first front (a stalled
        dependency); that step must fail with BOS_ERR_SOLVER and leave the state unchanged."""
        _check(lib().bos_debug_inject_stall(self._h), "bos_debug_inject_stall")

    def debug_solver_stamps(self, nsuper: int):
        """Diagnostics: one GN step with per-front stamps of the dataflow launches (bos_host.h)."""
        st = np.zeros((2, nsuper, 8), dtype=np.uint64)
        meta = np.zeros((nsuper, 4), dtype=np.int32)
        _check(lib().bos_debug_solver_stamps(self._h, st.size, st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                             meta.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "solver stamps")
        return st, meta

    # bos_host.h BOS_ROUTE_F_* / BOS_ROUTE_B_*, by value
    FACTOR_ROUTES = ("reg16", "reg16_side", "pan48", "pan64", "pan64_side", "blk", "blk_side2", "mixb_blk",
                     "mixb_wave", "level", "flow", "folded")
    BACKWARD_ROUTES = ("backward_flow", "backward_wave", "backward_level", "backward_fold")

    def debug_solver_routes(self) -> np.ndarray:
        """Diagnostics: [nsuper, 4] = factor route (FACTOR_ROUTES index), backward route
        (BACKWARD_ROUTES index), k, r of every front, as the launch sites noted them when the handle's
        first step was enqueued (bos_host.h bos_debug_solver_routes; BosError before that step)."""
        n = ctypes.c_int32(0)
        _check(lib().bos_debug_solver_routes(self._h, 0, None, ctypes.byref(n)), "bos_debug_solver_routes")
        out = np.zeros((n.value, 4), dtype=np.int32)
        _check(lib().bos_debug_solver_routes(self._h, out.size, _ptr(out, ctypes.c_int32), ctypes.byref(n)),
               "bos_debug_solver_routes")
        return out

    # bos_host.h BOS_SELINV_*, by value, and the columns of debug_selinv_fronts()["fronts"]
    SELINV_CLASSES = ("wave_lds", "blk_lds_mfma", "blk_workspace")
    SELINV_COLS = ("class", "launch", "k", "r", "folded", "sigma_front", "diag_records", "cross_rj", "cross_jj",
                   "cross_transposed")

    def debug_selinv_fronts(self) -> dict:
        """Diagnostics: what the selected inverse's launch plan decided (bos_host.h
        bos_debug_selinv_fronts; BosError before the handle's first marginals() / edge_covariances()).
        "fronts": [nsuper, 10] int32 with the columns SELINV_COLS (class = SELINV_CLASSES index; the
        three cross columns are -1 until edge_covariances() has built the cross records);
        "node_front": [NP + NL] the front that writes each node's block (-1: the fixed pose);
        "edge_front": [Mb + Mo] the front that emits each edge's cross block (bearings, then odometry;
        -1: the edge involves the fixed pose, or no cross records yet)."""
        n = ctypes.c_int32(0)
        _check(lib().bos_debug_selinv_fronts(self._h, 0, None, ctypes.byref(n), None, None), "bos_debug_selinv_fronts")
        fronts = np.zeros((n.value, len(self.SELINV_COLS)), dtype=np.int32)
        node = np.zeros(self.P.NP + self.P.NL, dtype=np.int32)
        edge = np.zeros(len(self.P.b_z) + len(self.P.o_z), dtype=np.int32)
        _check(lib().bos_debug_selinv_fronts(self._h, fronts.size, _ptr(fronts, ctypes.c_int32), ctypes.byref(n),
                                             _ptr(node, ctypes.c_int32), _ptr(edge, ctypes.c_int32)),
               "bos_debug_selinv_fronts")
        return {"fronts": fronts, "node_front": node, "edge_front": edge}

    def debug_set_step_graph(self, enable: bool):
        """Test hook: GN steps as individual launches (False) or the captured graph (True, default)."""
        _check(lib().bos_debug_set_step_graph(self._h, int(enable)), "bos_debug_set_step_graph")

    def time_linearize(self, n: int, flush_caches: bool = False) -> float:
        """ms per J+H build (HIP events on the handle's stream, see bos_time_linearize)."""
        ms = ctypes.c_double(0)
        _check(lib().bos_time_linearize(self._h, n, int(flush_caches), ctypes.byref(ms)), "bos_time_linearize")
        return ms.value

    def time_steps(self, n: int) -> float:
        """ms per synchronous GN iteration over n bos_step calls made from C (bos_time_steps)."""
        ms = ctypes.c_double(0)
        _check(lib().bos_time_steps(self._h, n, ctypes.byref(ms)), "bos_time_steps")
        return ms.value

    def time_triangulate(self, n: int) -> float:
        ms = ctypes.c_double(0)
        _check(lib().bos_time_triangulate(self._h, n, ctypes.byref(ms)), "bos_time_triangulate")
        return ms.value

    def triangulate(self):
        """triangulate_landmarks on the device from the current poses (slam/triangulation.cpp:65-74)."""
        _check(lib().bos_triangulate(self._h), "bos_triangulate")

    def triangulate_async(self):
        _check(lib().bos_triangulate_async(self._h), "bos_triangulate_async")

    def synchronize(self):
        _check(lib().bos_synchronize(self._h), "bos_synchronize")

    def system_info(self) -> dict:
        info = bos_system_info()
        _check(lib().bos_system_info_get(self._h, ctypes.byref(info)), "system_info")
        return {k: getattr(info, k) for k, _ in info._fields_}

    def export_system(self):
        """(rows, cols, vals, b): lower triangle of H_nf in reference dof numbering + full b."""
        info = self.system_info()
        nnz = info["nnz_lower"]
        rows = np.zeros(nnz, dtype=np.int32)
        cols = np.zeros(nnz, dtype=np.int32)
        vals = np.zeros(nnz)
        b = np.zeros(self.P.N)
        _check(lib().bos_export_system(self._h, nnz, _ptr(rows, ctypes.c_int32), _ptr(cols, ctypes.c_int32),
                                       _ptr(vals, ctypes.c_double), _ptr(b, ctypes.c_double)), "export_system")
        return rows, cols, vals, b

    def marginals(self, poses: bool = True, landmarks: bool = True):
        """Marginal covariances of the current estimate (bos_marginals): (pose_cov [NP, 3, 3],
        lm_cov [NL, 2, 2], solver_info); poses / landmarks False: that output is not asked for (None)."""
        pose = np.zeros((self.P.NP, 3, 3)) if poses else None
        lm = np.zeros((self.P.NL, 2, 2)) if landmarks else None
        info = ctypes.c_int32(0)
        _check(lib().bos_marginals(self._h, _ptr(pose, ctypes.c_double), _ptr(lm, ctypes.c_double),
                                   ctypes.byref(info)), "bos_marginals")
        return pose, lm, info.value

    def edge_covariances(self, cross: bool = True, projected: bool = True, blocks: bool = True) -> dict:
        """Edge covariances of the current estimate (bos_edge_covariances): a dict with bearing_cross
        [Mb, 3, 2] and odom_cross [Mo, 3, 3] (cross), bearing_var [Mb] and odom_cov [Mo, 3, 3]
        (projected), pose_cov [NP, 3, 3] and landmark_cov [NL, 2, 2] (blocks), and solver_info; outputs
        that were not asked for are None."""
        out = _edge_cov_arrays(self.P, cross, projected, blocks)
        info = ctypes.c_int32(0)
        _check(lib().bos_edge_covariances(self._h, *[_ptr(out[k], ctypes.c_double) for k in _EDGE_COV_ORDER],
                                          ctypes.byref(info)), "bos_edge_covariances")
        out["solver_info"] = info.value
        return out

    def _timing(self, fn: str, slots: tuple, bytes_key: str, *more) -> dict:
        """A covariance call's timing getter `fn`(handle, ms, bytes, *more): its ms slots under the names
        `slots`, in order, then the device bytes under `bytes_key`."""
        ms = np.zeros(len(slots))
        nb = ctypes.c_int64(0)
        _check(getattr(lib(), fn)(self._h, _ptr(ms, ctypes.c_double), ctypes.byref(nb), *more), fn)
        return {**dict(zip(slots, ms)), bytes_key: nb.value}

    def edge_covariances_timing(self) -> dict:
        """The last edge_covariances() call's split in ms and the feature's device bytes
        (bos_edge_covariances_timing)."""
        return self._timing("bos_edge_covariances_timing", ("jh_ms", "factor_ms", "selinv_ms", "project_ms", "download_ms"),
                            "edge_bytes")

    def edge_consistency(self, gate_bearing: float = 0.0, gate_odom: float = 0.0, k: int = 4, rows: bool = False, lists: bool = True,
                         kinds=("bearing", "odom")) -> dict:
        """Tests the edges that are in the graph against the current estimate (bos_edge_consistency): per kind
        the k largest normalised residuals w2 = e^T (Omega^-1 - J Sigma J^T)^-1 e at or above the gate,
        descending: cand_bearing / cand_odom [k] (edge index, -1 padding), cand_*_w2 [k] (-inf padding),
        cand_bearing_innovation / _resvar [k], cand_odom_innovation [k, 3], cand_odom_rescov [k, 3, 3] and the
        counts n_over_*; with rows the whole bearing_/odom_ w2, chi2 and redundancy arrays. Outputs not asked
        for (rows, lists, a kind not in kinds) are None. Includes solver_info."""
        out = _edge_check_arrays(self.P, k, lists, rows, kinds)
        info = ctypes.c_int32(0)
        _check(lib().bos_edge_consistency(self._h, gate_bearing, gate_odom, k, *_edge_check_pointers(out), ctypes.byref(info)),
               "bos_edge_consistency")
        out = _edge_check_result(out)
        out["solver_info"] = info.value
        return out

    def edge_consistency_timing(self) -> dict:
        """The last edge_consistency() call's split in ms and the feature's device bytes
        (bos_edge_consistency_timing)."""
        return self._timing("bos_edge_consistency_timing", ("host_ms", "jh_ms", "factor_ms", "selinv_ms", "score_ms", "select_ms",
                                                            "download_ms"), "bytes")

    def pair_covariances(self, node_a, node_b, cross: bool = True, projected: bool = True, blocks: bool = True) -> dict:
        """Joint covariances of arbitrary node pairs at the current estimate (bos_pair_covariances). Node
        ids: pose stix u is u, landmark stix l is NP + l; a mixed pair is (pose, landmark). Returns a dict
        of [n, 9] arrays, pair q's block row-major in the first rows * cols entries of row q (pair_block):
        cross, projected, cov_a and cov_b (blocks), and solver_info; outputs not asked for are None."""
        a, b, out = _pair_cov_arrays(node_a, node_b, cross, projected, blocks)
        info = ctypes.c_int32(0)
        _check(lib().bos_pair_covariances(self._h, len(a), _ptr(a, ctypes.c_int32), _ptr(b, ctypes.c_int32),
                                          *[_ptr(out[k], ctypes.c_double) for k in _PAIR_COV_ORDER], ctypes.byref(info)),
               "bos_pair_covariances")
        out["solver_info"] = info.value
        return out

    def pair_covariances_timing(self) -> dict:
        """The last pair_covariances() call's split in ms and the feature's device bytes
        (bos_pair_covariances_timing)."""
        return self._timing("bos_pair_covariances_timing",
                            ("prepare_ms", "jh_ms", "factor_ms", "path_ms", "product_ms", "download_ms"), "pair_bytes")

    def node_covariances(self, nodes, cross: bool = True, projected: bool = True, marginals: bool = False) -> dict:
        """One node's covariance against every node, for each node of `nodes`, at the current estimate
        (bos_node_covariances). Node ids: pose stix u is u, landmark stix l is NP + l. Returns a dict with
        cross_pose [n, NP, 9] and cross_landmark [n, NL, 6] (cross: Sigma(a, u), rows a's dofs, row-major in
        the first rows * cols entries of a slot), projected_pose [n, NP, 9] and projected_landmark [n, NL, 4]
        (projected), pose_cov [NP, 3, 3] and landmark_cov [NL, 2, 2] (marginals), and solver_info; outputs not
        asked for are None."""
        a, out = _node_cov_arrays(self.P, nodes, cross, projected, marginals)
        info = ctypes.c_int32(0)
        _check(lib().bos_node_covariances(self._h, len(a), _ptr(a, ctypes.c_int32),
                                          *[_ptr(out[k], ctypes.c_double) for k in _NODE_COV_ORDER], ctypes.byref(info)),
               "bos_node_covariances")
        out["solver_info"] = info.value
        return out

    def node_covariances_timing(self) -> dict:
        """The last node_covariances() call's split in ms and the feature's device bytes
        (bos_node_covariances_timing)."""
        return self._timing("bos_node_covariances_timing",
                            ("prepare_ms", "jh_ms", "factor_ms", "selinv_ms", "column_ms", "gather_ms", "download_ms"), "node_bytes")

    def associate_bearings(self, pose, z, omega=None, gate: float = np.inf, k: int = 4, nis_all: bool = False) -> dict:
        """Gates new bearings against every landmark at the current estimate (bos_associate_bearings):
        bearing q was measured as z[q] from pose stix pose[q] with information omega[q] (None: 1). Returns
        a dict with cand_landmark [n, k] (landmark stix, -1 padding), cand_nis [n, k] (+inf padding),
        cand_innovation and cand_var [n, k] (e and S = var + 1 / omega of the listed landmark, 0 padding),
        n_inside [n] (every landmark with nis <= gate), nis_all [n, NL] or None, and solver_info. The
        listed landmarks are the k smallest NIS inside the gate, ascending by (nis, stix)."""
        a, zz, om, out = _assoc_arrays(self.P, pose, z, omega, k, nis_all)
        info = ctypes.c_int32(0)
        _check(lib().bos_associate_bearings(self._h, len(a), _ptr(a, ctypes.c_int32), _ptr(zz, ctypes.c_double),
                                            _ptr(om, ctypes.c_double), gate, k, *_assoc_ptrs(out), ctypes.byref(info)),
               "bos_associate_bearings")
        out["solver_info"] = info.value
        return out

    def associate_bearings_timing(self) -> dict:
        """The last associate_bearings() call's split in ms and the feature's device bytes
        (bos_associate_bearings_timing)."""
        return self._timing("bos_associate_bearings_timing",
                            ("prepare_ms", "jh_ms", "factor_ms", "selinv_ms", "column_ms", "nis_ms", "select_ms", "download_ms"),
                            "assoc_bytes")

    def debug_set_associate_chunk(self, max_bearings: int):
        """Test knob (bos_debug_set_associate_chunk): associate_bearings() closes a chunk at this many
        bearings of one pose; 0 restores the byte budget."""
        _check(lib().bos_debug_set_associate_chunk(self._h, max_bearings), "bos_debug_set_associate_chunk")

    def joint_compatibility(self, hypotheses, z=None, omega=None, cov: bool = False) -> dict:
        """Joint compatibility of association hypotheses at the current estimate (bos_joint_compatibility):
        the joint NIS e^T (J Sigma J^T + R)^-1 e over the stacked innovation of each hypothesis of at most
        JOINT_MAX_M pairings (bearing z from pose stix `pose` assigned to landmark stix `landmark`,
        information omega, None: 1). `hypotheses` is a list of (pose, landmark, z[, omega]) arrays, one tuple
        per hypothesis; or, with the flat z (and omega) given, the tuple (hyp_start, pose, landmark). Returns
        a dict with prefix_nis [n_pair] (entry i of a hypothesis: the joint NIS of its pairings 0 .. i),
        joint_nis [n_hyp] (0 for an empty hypothesis), innovation [n_pair], innovation_cov (cov: a list of
        m x m arrays; else None), hyp_start and solver_info."""
        start, a, l, zz, om, out = _joint_arrays(hypotheses, z, omega, cov)
        info = ctypes.c_int32(0)
        _check(lib().bos_joint_compatibility(self._h, len(start) - 1, _ptr(start, ctypes.c_int32), _ptr(a, ctypes.c_int32),
                                             _ptr(l, ctypes.c_int32), _ptr(zz, ctypes.c_double), _ptr(om, ctypes.c_double),
                                             *[_ptr(out[k], ctypes.c_double) for k in _JOINT_ORDER], ctypes.byref(info)),
               "bos_joint_compatibility")
        out["solver_info"] = info.value
        return _joint_finish(start, out)

    def joint_compatibility_timing(self) -> dict:
        """The last joint_compatibility() call's split in ms and the device bytes it uses
        (bos_joint_compatibility_timing)."""
        return self._timing("bos_joint_compatibility_timing",
                            ("prepare_ms", "jh_ms", "factor_ms", "path_ms", "product_ms", "nis_ms", "download_ms"), "joint_bytes")

    def debug_set_joint_batch(self, max_hypotheses: int):
        """Test knob (bos_debug_set_joint_batch): joint_compatibility() closes a batch at this many
        hypotheses; 0 restores the budgets."""
        _check(lib().bos_debug_set_joint_batch(self._h, max_hypotheses), "bos_debug_set_joint_batch")

    def jcbb(self, frames, gate, max_nodes: int = 0, cov: bool = False, detail: bool = True) -> dict:
        """Joint-compatibility branch and bound at the current estimate (bos_jcbb): per frame of at most
        JCBB_MAX_BEARINGS new bearings with candidate lists (at most JOINT_MAX_M pairings), the admissible
        hypothesis with the most pairings, then the smallest joint NIS, then the lexicographically smallest
        choice vector, searched on the device. `frames` is a list of (pose, z, omega_or_None, candidates), one
        tuple per frame; candidates is a list of lists or a 2-D array with -1 padding such as
        associate_bearings()["cand_landmark"]. gate [JOINT_MAX_M]: chi^2 quantiles by degrees of freedom.
        max_nodes: the node budget per frame (0: 2^22). Returns a dict with assignment [n_bearings] (landmark
        stix or -1), n_paired, joint_nis, complete [n_frames], prefix_nis [n_bearings], innovation [n_pairings],
        innovation_cov (cov: a list of P x P arrays; else None), frame_start, cand_start, cand_landmark and
        solver_info. detail False: the assignment alone is computed (the other outputs are None)."""
        a, out = _jcbb_arrays(frames, gate, cov, detail)
        info = ctypes.c_int32(0)
        _check(lib().bos_jcbb(self._h, len(a["frame_start"]) - 1, _ptr(a["frame_start"], ctypes.c_int32),
                              _ptr(a["pose"], ctypes.c_int32), _ptr(a["z"], ctypes.c_double), _ptr(a["omega"], ctypes.c_double),
                              _ptr(a["cand_start"], ctypes.c_int32), _ptr(a["cand_landmark"], ctypes.c_int32),
                              _ptr(a["gate"], ctypes.c_double), max_nodes, *_jcbb_out_ptrs(out), ctypes.byref(info)),
               "bos_jcbb")
        out["solver_info"] = info.value
        return _jcbb_finish(a, out)

    def jcbb_timing(self) -> dict:
        """The last jcbb() call's split in ms, the device bytes it uses and the nodes its search visited per
        frame (bos_jcbb_timing)."""
        slots = ("prepare_ms", "jh_ms", "factor_ms", "path_ms", "product_ms", "search_ms", "download_ms")
        nf = ctypes.c_int32(0)
        self._timing("bos_jcbb_timing", slots, "jcbb_bytes", 0, None, ctypes.byref(nf))
        nodes = np.zeros(max(nf.value, 1), dtype=np.int64)
        out = self._timing("bos_jcbb_timing", slots, "jcbb_bytes", nf.value, _ptr(nodes, ctypes.c_int64), None)
        out["nodes"] = nodes[:nf.value]
        return out

    def debug_set_jcbb_batch(self, max_frames: int):
        """Test knob (bos_debug_set_jcbb_batch): jcbb() closes a batch at this many frames; 0 restores the
        budgets."""
        _check(lib().bos_debug_set_jcbb_batch(self._h, max_frames), "bos_debug_set_jcbb_batch")

    def match_landmarks(self, landmarks, gate: float = np.inf, k: int = 4, d2_all: bool = False) -> dict:
        """Gates each query landmark against every other landmark at the current estimate
        (bos_match_landmarks). Returns a dict with cand_landmark [n, k] (stix, -1 padding), cand_d2 [n, k]
        (+inf padding), cand_diff [n, k, 2] and cand_cov [n, k, 4] (d = l_a - l_l and its covariance C, 0
        padding), n_inside [n] (every landmark with d2 <= gate), d2_all [n, NL] or None (NaN at the query
        itself), and solver_info. The listed landmarks are the k smallest d2 inside the gate, ascending by
        (d2, stix)."""
        a, out = _match_lm_arrays(self.P, landmarks, k, d2_all)
        info = ctypes.c_int32(0)
        _check(lib().bos_match_landmarks(self._h, len(a), _ptr(a, ctypes.c_int32), gate, k, *_match_ptrs(out, _MATCH_LM_ORDER),
                                         ctypes.byref(info)),
               "bos_match_landmarks")
        out["solver_info"] = info.value
        return out

    def match_poses(self, pose, z, omega=None, gate: float = np.inf, k: int = 4, nis_all: bool = False) -> dict:
        """Gates relative-pose measurements against every pose at the current estimate (bos_match_poses):
        measurement q is z[q] = (x, y, theta) in the frame of pose stix pose[q] with the 3 x 3 information
        omega[q] (None: the identity; one 3 x 3 matrix serves every measurement). Returns a dict with
        cand_pose [n, k] (stix, -1 padding), cand_nis [n, k] (+inf padding), cand_innovation [n, k, 3] and
        cand_cov [n, k, 9] (e and S = P + omega^-1 of the listed pose, 0 padding), n_inside [n], nis_all
        [n, NP] or None, and solver_info."""
        a, zz, om, out = _match_pose_arrays(self.P, pose, z, omega, k, nis_all)
        info = ctypes.c_int32(0)
        _check(lib().bos_match_poses(self._h, len(a), _ptr(a, ctypes.c_int32), _ptr(zz, ctypes.c_double), _ptr(om, ctypes.c_double),
                                     gate, k, *_match_ptrs(out, _MATCH_POSE_ORDER), ctypes.byref(info)),
               "bos_match_poses")
        out["solver_info"] = info.value
        return out

    def match_timing(self) -> dict:
        """The split in ms of the last match_landmarks() or match_poses() call and the feature's device
        bytes (bos_match_timing)."""
        return self._timing("bos_match_timing",
                            ("prepare_ms", "jh_ms", "factor_ms", "selinv_ms", "column_ms", "score_ms", "select_ms", "download_ms"),
                            "match_bytes")

    def debug_set_match_chunk(self, max_rows: int):
        """Test knob (bos_debug_set_match_chunk): match_poses() closes a chunk at this many measurements
        of one pose; 0 restores the byte budget."""
        _check(lib().bos_debug_set_match_chunk(self._h, max_rows), "bos_debug_set_match_chunk")

    def debug_set_pair_batch(self, max_distinct_nodes: int):
        """Test knob (bos_debug_set_pair_batch): pair_covariances() closes a batch at this many distinct
        nodes; 0 restores the byte budget."""
        _check(lib().bos_debug_set_pair_batch(self._h, max_distinct_nodes), "bos_debug_set_pair_batch")

    def cost(self) -> dict:
        """The objective F at the current state, the plain chi2 and the count of edges beyond the
        kernel threshold (bos_cost; fp64 on every handle, no H is built)."""
        return _run_cost(lib().bos_cost, self._h, "bos_cost")

    def optimize(self, **opts) -> dict:
        """Levenberg-Marquardt with on-device step control (bos_optimize). opts: the fields of
        bos_lm_options (lambda0, lambda_min, lambda_max, dx_tol, f_tol, max_iterations, check_every).
        Returns the bos_lm_result fields plus "trace": one LM_TRACE_DTYPE record per iteration."""
        return _run_optimize(lib().bos_optimize, self._h, "bos_optimize", opts)

    def time_cost(self, n: int) -> float:
        """ms per launch of the cost kernel (HIP events, bos_time_cost)."""
        ms = ctypes.c_double(0)
        _check(lib().bos_time_cost(self._h, n, ctypes.byref(ms)), "bos_time_cost")
        return ms.value

    def marginals_timing(self) -> dict:
        """The last marginals() call's split in ms and the Sigma-front buffer's bytes (bos_marginals_timing)."""
        return self._timing("bos_marginals_timing", ("jh_ms", "factor_ms", "selinv_ms", "download_ms"), "sigma_bytes")

    def get_state(self):
        pose = np.zeros((self.P.NP, 3))
        lm = np.zeros((self.P.NL, 2))
        _check(lib().bos_get_state(self._h, _ptr(pose, ctypes.c_double), _ptr(lm, ctypes.c_double)), "get_state")
        return pose, lm

    def set_state(self, pose_xyt, lm_xy):
        pose = np.ascontiguousarray(pose_xyt, dtype=np.float64)
        lm = np.ascontiguousarray(lm_xy, dtype=np.float64)
        _check(lib().bos_set_state(self._h, _ptr(pose, ctypes.c_double), _ptr(lm, ctypes.c_double)), "set_state")

    def last_dx(self):
        dx = np.zeros(self.P.N)
        _check(lib().bos_get_last_dx(self._h, _ptr(dx, ctypes.c_double)), "get_last_dx")
        return dx

    @property
    def state(self):
        return self.get_state()
