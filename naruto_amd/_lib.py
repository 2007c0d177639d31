"""ctypes binding of libnaruto_hip.so (C ABI: include/naruto_hip.h).

This is the ONLY compute backend of the package: if the shared library has not been built the import
fails loudly -- there is no PyTorch / CPU fallback for the hot path.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NARUTO_HIP_LIB") or os.path.join(_HERE, "libnaruto_hip.so")      # override: kernel experiments only
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["naruto_api.hip", "naruto_field.hip", "naruto_binned.hip", "naruto_render.hip", "naruto_rays.hip", "naruto_train.hip", "naruto_renderfused.hip", "naruto_planner.hip", "naruto_mesh.hip", "naruto_parts.hip",
           "naruto_sorted.hip", "naruto_pointgrad.hip", "naruto_track.hip", "naruto_bapose.hip", "naruto_rrt.hip", "naruto_recon.hip", "naruto_cull.hip", "naruto_subdiv.hip", "naruto_sim.hip", "naruto_frame.hip", "naruto_posechain.hip", "naruto_icp.hip", "naruto_view.hip", "naruto_icp.h", "naruto_pose.h", "naruto_mc_table.inc", "naruto_common.h"]
HEADER = os.path.join(os.path.dirname(_HERE), "include", "naruto_hip.h")

MAX_LEVELS = 16
LOSS_NSUMS = 16
LOSS_SLOT_MINUNCERT = 9


class NarutoFieldDesc(C.Structure):
    _fields_ = [
        ("n_levels", C.c_uint32), ("n_features", C.c_uint32), ("log2_hashmap_size", C.c_uint32),
        ("base_resolution", C.c_uint32), ("per_level_scale", C.c_float), ("n_bins", C.c_uint32),
        ("hidden_dim", C.c_uint32), ("geo_feat_dim", C.c_uint32), ("hidden_dim_color", C.c_uint32),
        ("uncert_dims", C.c_uint32 * 3), ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3),
        ("trunc", C.c_float), ("sc_factor", C.c_float), ("white_bkgd", C.c_int32), ("mlp_mode", C.c_uint32),
    ]


class NarutoParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("table", "uncert_grid", "sdf_w0", "sdf_w1", "col_w0", "col_w1")]


class NarutoGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("table", "uncert_grid", "sdf_w0", "sdf_w1", "col_w0", "col_w1")]


class NarutoExtraPoints(C.Structure):
    _fields_ = [("x", C.c_void_p), ("d_feat", C.c_void_p), ("scale", C.c_void_p), ("n", C.c_uint32)]


class NarutoAdamSeg(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_uint64), ("lr", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("step_lag", C.c_uint32)]


MLP_FP32, MLP_BF16 = 0, 1
BWD_OVERWRITE_WEIGHT_GRADS = 1
BWD_OVERWRITE_TABLE_GRAD = 2
BWD_POINTS_ACCUMULATE = 1
TRAIN_BWD_MLP_ONLY, TRAIN_BWD_TABLE_ONLY = 4, 8
TRAIN_FWD_DEFER_TAIL, TRAIN_BWD_DEFERRED_TAIL, TRAIN_BWD_SUMS_GIVEN = 2, 16, 32
TRAIN_FWD_SUMS_TV_LATER, TRAIN_BWD_TV_MOVED = 3, 64
ADAM_ADVANCE = 1
ADAM_ZERO_GRAD = 2


class NarutoRayBatch(C.Structure):
    _fields_ = [("store", C.c_void_p), ("n_kf", C.c_uint32), ("rays_per_kf", C.c_uint32), ("frame_ids", C.c_void_p),
                ("keyframe_every", C.c_int64), ("n_global", C.c_uint32), ("current", C.c_void_p), ("cur_list", C.c_void_p),
                ("n_cur_pop", C.c_uint64), ("n_cur", C.c_uint32), ("poses", C.c_void_p), ("n_poses", C.c_uint32),
                ("seed", C.c_uint64), ("counter", C.c_uint64), ("rays_o", C.c_void_p), ("rays_d", C.c_void_p),
                ("target_s", C.c_void_p), ("target_d", C.c_void_p), ("ids_out", C.c_void_p), ("rng", C.c_void_p), ("dyn", C.c_void_p),
                ("keys_out", C.c_void_p), ("key_base", C.c_uint32), ("key_tail", C.c_uint32), ("key_vol", C.c_void_p), ("key_dims", C.c_uint32 * 3),
                ("key_bbox_min", C.c_float * 3), ("key_voxel_scale", C.c_float)]


class NarutoFusedAdam(C.Structure):
    _fields_ = [("param", C.c_void_p * 5), ("exp_avg", C.c_void_p * 5), ("exp_avg_sq", C.c_void_p * 5),
                ("lr", C.c_float * 5), ("eps", C.c_float * 5), ("weight_decay", C.c_float * 5),
                ("beta1", C.c_float), ("beta2", C.c_float), ("step_dev", C.c_void_p), ("next_batch", C.c_void_p),
                ("uncert_step", C.c_uint32), ("uncert_step_lag", C.c_uint32), ("uncert_exp_avg", C.c_void_p), ("uncert_exp_avg_sq", C.c_void_p),
                ("uncert_step_dev", C.c_void_p), ("uncert_lr", C.c_float), ("uncert_eps", C.c_float), ("uncert_weight_decay", C.c_float),
                ("uncert_beta1", C.c_float), ("uncert_beta2", C.c_float)]


class NarutoTrainStep(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint32), ("n_samples_d", C.c_uint32), ("n_range_d", C.c_uint32), ("perturb", C.c_uint32),
        ("near_", C.c_float), ("far_", C.c_float), ("range_d", C.c_float), ("depth_trunc", C.c_float), ("rgb_missing", C.c_float),
        ("smooth_points", C.c_uint32), ("smooth_voxel", C.c_float), ("smooth_margin", C.c_float), ("smooth_grad_scale", C.c_float),
        ("n_rays_total", C.c_uint64),
        ("rays_o", C.c_void_p), ("rays_d", C.c_void_p), ("target_rgb", C.c_void_p), ("target_d", C.c_void_p),
        ("rand", C.c_void_p), ("rand6", C.c_void_p), ("rng", C.c_void_p), ("loss_weights", C.c_void_p),
        ("z_vals", C.c_void_p), ("raw", C.c_void_p), ("feat_save", C.c_void_p),
        ("rgb", C.c_void_p), ("depth", C.c_void_p), ("uncert_map", C.c_void_p),
        ("sums", C.c_void_p), ("losses", C.c_void_p), ("d_raw", C.c_void_p),
        ("ray_count", C.c_void_p), ("ray_offset", C.c_void_p), ("active_idx", C.c_void_p), ("n_active", C.c_void_p),
        ("workspace", C.c_void_p), ("loss_weight_parts", C.c_void_p * 10), ("min_uncert_running", C.c_void_p),
        ("fwd_image", C.c_void_p), ("fwd_image_fresh", C.c_uint32),
    ]


class NarutoTrackStep(C.Structure):
    _fields_ = [
        ("n_rays", C.c_uint32), ("H", C.c_uint32), ("W", C.c_uint32), ("edge_h", C.c_uint32), ("edge_w", C.c_uint32),
        ("direction", C.c_void_p), ("rgb", C.c_void_p), ("depth", C.c_void_p), ("rng", C.c_void_p),
        ("d_cam", C.c_void_p), ("pix", C.c_void_p), ("pose_init", C.c_void_p),
        ("pose", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("state", C.c_void_p),
        ("lr_rot", C.c_float), ("lr_trans", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("wait_iters", C.c_uint32), ("best", C.c_int32),
        ("best_pose", C.c_void_p), ("best_loss", C.c_void_p), ("c2w", C.c_void_p), ("d_rays_o", C.c_void_p), ("d_rays_d", C.c_void_p),
        ("trace_loss", C.c_void_p), ("trace_pose", C.c_void_p), ("trace_d_pose", C.c_void_p), ("max_trace", C.c_uint32),
        ("workspace", C.c_void_p),
    ]


class NarutoBAPoses(C.Structure):
    _fields_ = [
        ("max_poses", C.c_uint32), ("optim_cur", C.c_uint32), ("pose_accum_step", C.c_uint32), ("dyn", C.c_void_p),
        ("poses", C.c_void_p), ("pose_init", C.c_void_p), ("pose6", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
        ("accum", C.c_void_p), ("state", C.c_void_p), ("ids", C.c_void_p), ("n_ids", C.c_uint32), ("src_rows", C.c_void_p),
        ("d_rays_o", C.c_void_p), ("d_rays_d", C.c_void_p),
        ("lr_rot", C.c_float), ("lr_trans", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
        ("trace_pose", C.c_void_p), ("trace_grad", C.c_void_p), ("max_trace", C.c_uint32), ("workspace", C.c_void_p),
    ]


class NarutoRrtPlan(C.Structure):
    _fields_ = [("dims", C.c_uint32 * 3), ("range", (C.c_double * 2) * 3), ("full_range", (C.c_double * 2) * 3),
                ("step_size", C.c_double), ("step_amplifier", C.c_double), ("collision_thre", C.c_double), ("enable_direct_line", C.c_int32),
                ("sdf_vol", C.c_void_p), ("workspace", C.c_void_p), ("nodes_xyz", C.c_void_p), ("nodes_xyz32", C.c_void_p),
                ("parent", C.c_void_p), ("next", C.c_void_p), ("capacity", C.c_uint32), ("cell_threshold", C.c_uint32)]


class NarutoNnGrid(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("dims", C.c_uint32 * 3), ("lo", C.c_double * 3), ("cell", C.c_double),
                ("cell_start", C.c_void_p), ("points", C.c_void_p)]


class NarutoCullCam(C.Structure):
    _fields_ = [("H", C.c_uint32), ("W", C.c_uint32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_", C.c_float), ("far_", C.c_float)]


ICP_SUMS = 17                            # count, sum d^2, sum p [3], sum q [3], sum p q^T [9]
ICP_STATE_DOUBLES = 24                   # T [16], fitness, inlier_rmse, previous fitness, previous rmse, iteration, status, s2 / s1, 0
ICP_RUNNING, ICP_CONVERGED, ICP_DEGENERATE, ICP_MAX_ITERATION = range(4)
ICP_STATUS = ("running", "converged", "degenerate", "max_iteration")

SIM_KEEP_INF = 1

GOAL_SEARCH_HEAD_INTS = 8                # naruto_goal_search's out: int32 head[8], then 11 four-byte words per look-at slot
GOAL_SEARCH_MAX_TARGETS = 4096

RRT_MODE_RUN, RRT_MODE_FULL = 0, 1
RRT_DONE, RRT_NEED_ROWS, RRT_NEED_ROOM = 0, 1, 2
RRT_CELL_THRESHOLD = 2048
RRT_STATE_NODES, RRT_STATE_ITER, RRT_STATE_RRT_ITER, RRT_STATE_STATUS, RRT_STATE_ROWS_USED, RRT_STATE_GOAL_PARENT, RRT_STATE_REACHABLE = range(7)
RRT_STATE_MID_ITER, RRT_STATE_USE_CELLS = 7, 9
RRT_STATE_INTS = 16


class NarutoRender(C.Structure):
    _fields_ = [("n_rays", C.c_uint32), ("rays_o", C.c_void_p), ("rays_d", C.c_void_p), ("target_d", C.c_void_p),
                ("near_", C.c_float), ("far_", C.c_float), ("n_samples_d", C.c_uint32), ("n_range_d", C.c_uint32), ("range_d", C.c_float),
                ("n_samples", C.c_uint32), ("rand", C.c_void_p), ("rng", C.c_void_p),
                ("rgb", C.c_void_p), ("depth", C.c_void_p), ("disp", C.c_void_p), ("acc", C.c_void_p), ("depth_var", C.c_void_p),
                ("uncert_map", C.c_void_p), ("weights", C.c_void_p), ("raw", C.c_void_p), ("z_vals", C.c_void_p)]


class NarutoViewRender(C.Structure):
    _fields_ = [("n_poses", C.c_uint32), ("poses", C.c_void_p), ("p0", C.c_uint32), ("p1", C.c_uint32), ("target_d", C.c_void_p),
                ("n_samples_d", C.c_uint32), ("n_range_d", C.c_uint32), ("range_d", C.c_float), ("n_coarse", C.c_uint32),
                ("rgb", C.c_void_p), ("depth", C.c_void_p), ("acc", C.c_void_p), ("depth_var", C.c_void_p), ("uncert_map", C.c_void_p),
                ("surface_z", C.c_void_p)]


class NarutoPoints(C.Structure):
    _fields_ = [("x", C.c_void_p), ("rays_o", C.c_void_p), ("rays_d", C.c_void_p), ("z_vals", C.c_void_p),
                ("n_samples", C.c_uint32)]


def build_command(out: str = LIB_PATH) -> List[str]:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics",
            os.path.join(CSRC, "naruto_api.hip"), "-o", out]


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [HEADER]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or needs_build():
        tmp = f"{LIB_PATH}.{os.getpid()}.tmp"               # never a half-written library under the final name
        cmd = build_command(tmp)
        if verbose:
            print(" ".join(cmd))
        try:
            subprocess.run(cmd, check=True)
            os.replace(tmp, LIB_PATH)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return LIB_PATH


_V, _U32, _U64, _F, _I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float, C.c_int

# name -> (restype, argtypes); every symbol include/naruto_hip.h declares
SIGNATURES = {
    "naruto_last_error": (C.c_char_p, []),
    "naruto_version": (_I, []),
    "naruto_field_create": (_I, [C.POINTER(NarutoFieldDesc), C.POINTER(_V)]),
    "naruto_field_destroy": (None, [_V]),
    "naruto_field_levels": (_I, [_V, C.POINTER(_F), C.POINTER(_U32), C.POINTER(_U32), C.POINTER(_U32)]),
    "naruto_field_n_entries": (_U64, [_V]),
    "naruto_sample_z": (_I, [_U32, _V, _F, _F, _U32, _U32, _F, _U32, _V, _V, _V]),
    "naruto_hash_encode_fwd": (_I, [_V, _U32, _V, _V, _V, _V]),
    "naruto_scatter_workspace": (C.c_size_t, [_V, _U32]),
    "naruto_field_scatter_overwrites": (C.c_int, [_V]),
    "naruto_hash_encode_bwd": (_I, [_V, _U32, _V, _V, _V, _V, _V, _V]),
    "naruto_smoothness_workspace": (C.c_size_t, [_U32]),
    "naruto_smoothness_fwd": (_I, [_V, _V, _U32, _F, _F, _V, _V, _V, _V, _V, _V]),
    "naruto_query_fwd": (_I, [_V, C.POINTER(NarutoParams), _U32, C.POINTER(NarutoPoints), _V, _V, _V, _V, _V]),
    "naruto_query_bwd_workspace": (C.c_size_t, [_V, _U32]),
    "naruto_query_bwd": (_I, [_V, C.POINTER(NarutoParams), _U32, C.POINTER(NarutoPoints), _V, _V, _V, _V, _V,
                              C.POINTER(NarutoExtraPoints), _U32, C.POINTER(NarutoGrads), _V, _V]),
    "naruto_query_bwd_points_workspace": (C.c_size_t, [_V, _U32]),
    "naruto_query_bwd_points": (_I, [_V, C.POINTER(NarutoParams), _U32, C.POINTER(NarutoPoints), _V, _V, _V, _V, _V, _V, _V, _U32, _V, _V]),
    "naruto_active_ray_workspace": (C.c_size_t, [_U32, _U32]),
    "naruto_active_ray_select_keyed": (_I, [_U32, _U32, _U32, _U32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "naruto_active_ray_select": (_I, [_U32, _U32, _U32, _U32, _V, _V, _V, _V, _V, C.POINTER(_U32), C.POINTER(_F), _F, _V, _V, _V, _V, _V, _V]),
    "naruto_active_ray_select_keyed_rows": (_I, [_U32, _U32, _U32, _U32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "naruto_active_ray_select_rows": (_I, [_U32, _U32, _U32, _U32, _V, _V, _V, _V, _V, C.POINTER(_U32), C.POINTER(_F), _F, _V, _V, _V, _V, _V, _V, _V]),
    "naruto_rays_to_world": (_I, [_U32, _V, _V, _V, _V, _V, _V]),
    "naruto_map_volumes": (_I, [_U32, _V, _V, _V]),
    "naruto_assemble_rays": (_I, [C.POINTER(NarutoRayBatch), _V]),
    "naruto_assemble_select": (_I, [C.POINTER(NarutoRayBatch), _U32, _U32, _U32, _V, C.POINTER(_U32), C.POINTER(_F), _F, _V, _V, _V, _V, _V]),
    "naruto_sample_distinct": (_I, [_U64, _U32, _U64, _U64, _V, _V]),
    "naruto_perm_index": (_U64, [_U64, _U64, _U64, _U64, _U64]),
    "naruto_frame_ingest": (_I, [_U64, _V, _V, _V, _F, _V, _V, _V]),
    "naruto_keyframe_row": (_I, [_V, _U64, _V, _U32, _U64, _U64, _V, _V]),
    "naruto_pose_log": (_I, [_U32, _V, _V, _V]),
    "naruto_pose_predict": (_I, [_V, _U32, _U32, C.c_int32, _V, _V]),
    "naruto_pose_commit": (_I, [_V, _V, _U32, _U32, _U32, _V, _V]),
    "naruto_pose_scatter": (_I, [_V, _U32, _V, _U32, _U32, _U32, C.c_int32, _V]),
    "naruto_pose_resolve": (_I, [_V, _V, _U32, _U32, _V, _V]),
    "naruto_debug_pose_log": (_I, [_U32, _V, _V]),
    "naruto_goal_targets_workspace": (C.c_size_t, [_U32, _U32]),
    "naruto_goal_targets": (_I, [C.POINTER(_U32), _V, _U32, _U32, _V, _V, _V]),
    "naruto_goal_aggregate": (_I, [C.POINTER(_U32), _V, _V, _U32, _V, _U32, _V, _F, _F, _F, _V, _V, _V]),
    "naruto_goal_search": (_I, [_U32, _U32, _V, _V, _V, _V, _U32, C.POINTER(C.c_double), C.c_double, _V, _V]),
    "naruto_rrt_workspace": (C.c_size_t, [C.POINTER(_U32)]),
    "naruto_rrt_start": (_I, [C.POINTER(NarutoRrtPlan), C.POINTER(C.c_double), C.POINTER(C.c_double), _V]),
    "naruto_rrt_grow": (_I, [C.POINTER(NarutoRrtPlan), _I, _V, _U32, _U32, _I, _V]),
    "naruto_rrt_path": (_I, [C.POINTER(NarutoRrtPlan), _V, _V]),
    "naruto_segments_free": (_I, [C.POINTER(_U32), _V, _U32, _V, _V, C.c_double, C.c_double, _V, _V, _V]),
    "naruto_reachable_mask": (_I, [C.POINTER(NarutoRrtPlan), _V, _V]),
    "naruto_lattice_points": (_I, [C.POINTER(_U32), _V, _V, _V, _V, _V]),
    "naruto_mesh_workspace": (C.c_size_t, [C.POINTER(_U32)]),
    "naruto_mesh_count": (_I, [C.POINTER(_U32), _V, C.c_double, C.c_double, _V, _V, _V]),
    "naruto_mesh_emit": (_I, [C.POINTER(_U32), _V, C.c_double, _V, _U64, _U64, _V, _V, _V]),
    "naruto_surface_areas": (_I, [_U64, _U64, _V, _I, _V, _V, _V]),
    "naruto_surface_sample": (_I, [_U64, _U64, _V, _I, _V, _V, _U64, _U64, _V, _V, _V]),
    "naruto_nn_grid_plan": (_I, [_U64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, _U64, C.POINTER(NarutoNnGrid)]),
    "naruto_nn_grid_workspace": (C.c_size_t, [C.POINTER(NarutoNnGrid)]),
    "naruto_nn_grid_build": (_I, [C.POINTER(NarutoNnGrid), _V, _V, _V]),
    "naruto_nn_grid_query": (_I, [C.POINTER(NarutoNnGrid), _U64, _V, _V, _U32, _V, _V, _V, _V]),
    "naruto_nn_scan": (_I, [_U64, _V, _U64, _V, _V, _V, _V]),
    "naruto_dist_reduce_workspace": (C.c_size_t, [_U64]),
    "naruto_dist_reduce": (_I, [_U64, _V, C.c_double, _V, _V, _V]),
    "naruto_icp_transform": (_I, [_U64, _V, _I, _V, _V, _V]),
    "naruto_icp_accumulate_workspace": (C.c_size_t, [_U64]),
    "naruto_icp_accumulate": (_I, [_U64, _V, _U64, _V, _V, _V, C.c_double, C.POINTER(C.c_double), _V, _V, _V]),
    "naruto_icp_step": (_I, [_V, _U64, C.POINTER(C.c_double), _U32, C.c_double, C.c_double, _V, _V]),
    "naruto_debug_icp_solve": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "naruto_render_depth_workspace": (C.c_size_t, [_U64, _U64, _U32]),
    "naruto_render_depth": (_I, [C.POINTER(NarutoCullCam), _U64, _V, _U64, _V, _V, _U32, _V, _U32, _V, _V, _V]),
    "naruto_observed_vertices": (_I, [C.POINTER(NarutoCullCam), _U64, _V, _U32, _V, _V, _F, _V, _V]),
    "naruto_cull_faces": (_I, [_U64, _U64, _V, _V, _V, _V, _V, _V]),
    "naruto_cull_compact": (_I, [_U64, _U64, _V, _V, _V, _V, _V, _V, _I, _V, _U64, _U64, _V, _V, _V, _V]),
    "naruto_debug_atomic_min_rate": (_I, [_U64, _U32, _U32, _V, _V]),
    "naruto_subdivide_workspace": (C.c_size_t, [_U64, _U64]),
    "naruto_subdivide_mark": (_I, [_U64, _U64, _V, _V, _I, C.c_double, _V, _V]),
    "naruto_subdivide_edges": (_I, [_U64, _U64, _V, _V, _V, _U64, _U64, _V, _V, _V]),
    "naruto_subdivide_emit": (_I, [_U64, _U64, _V, _V, _V, _U64, _U64, _V, _V, _U64, _V, _I, _V, _V, _V]),
    "naruto_render_rgbd_workspace": (C.c_size_t, [_U64, _U64, _U32, _U32, _U32]),
    "naruto_render_rgbd": (_I, [C.POINTER(NarutoCullCam), _U64, _V, _U64, _V, _V, _I, _U32, _V, _U32, _U32, _V, _V, _V, _V, _V]),
    "naruto_cube_to_erp": (_I, [_U32, _U32, _U64, _V, _V, _V, _V]),
    "naruto_depth_to_dist": (_I, [_U32, _U32, _U32, _F, _F, _F, _F, _V, _V, _V]),
    "naruto_sim_erp": (_I, [_U32, _U32, _U64, _V, _V, _V, _F, _V, _V, _V, _V]),
    "naruto_debug_atomic_min64_rate": (_I, [_U64, _U32, _U32, _V, _V]),
    "naruto_view_rays": (_I, [C.POINTER(NarutoCullCam), _U32, _V, _U32, _U32, _V, _V, _V]),
    "naruto_view_crossing": (_I, [_U32, _U32, _V, _V, _V, _V]),
    "naruto_render_view": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoCullCam), C.POINTER(NarutoViewRender), _V]),
    "naruto_image_metrics_workspace": (C.c_size_t, [_U32, _U32, _U32]),
    "naruto_image_metrics": (_I, [_U32, _U32, _U32, _V, _V, _V, _V, _I, _F, C.POINTER(C.c_double), _V, _V, _V, _V, _V, _V]),
    "naruto_adam_multi": (_I, [C.POINTER(NarutoAdamSeg), _U32, _F, _F, _U32, _V, _U32, _V]),
    "naruto_train_workspace": (C.c_size_t, [_V, C.POINTER(NarutoTrainStep)]),
    "naruto_train_forward": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), _I, _V]),
    "naruto_train_finalize": (_I, [_V, C.POINTER(NarutoTrainStep), _V]),
    "naruto_oneblob_fwd": (_I, [_V, C.c_uint32, _V, _V, _V]),
    "naruto_uncert_sample": (_I, [_V, C.c_uint32, _V, _V, _V, _V]),
    "naruto_debug_random_lines": (_I, [_V, C.c_uint64, C.c_uint32, _V, C.POINTER(C.c_uint64), _V]),
    "naruto_decoder_fwd": (_I, [_V, C.POINTER(NarutoParams), C.c_uint32, C.c_int, _V, _V, _V, _V]),
    "naruto_debug_train_query_fwd": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), _V]),
    "naruto_debug_fwd_timeline": (_I, [_V]),
    "naruto_debug_bwd_timeline": (_I, [_V]),
    "naruto_debug_query_bwd_lds_bytes": (C.c_size_t, []),
    "naruto_fwd_image_bytes": (C.c_size_t, [C.POINTER(C.c_size_t), C.POINTER(_U32)]),
    "naruto_fwd_image_init": (_I, [_V, C.POINTER(NarutoParams), _V, _V]),
    "naruto_debug_fwd_image": (_I, [_V, C.POINTER(NarutoParams), _V, _V]),
    "naruto_debug_fwd_image_map": (_I, [_V, _V]),
    "naruto_debug_train_scatter": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), _V]),
    "naruto_debug_scatter_list": (_I, [_V, _U32, _V, _V, _V, _V, _V, _V]),
    "naruto_debug_train_plan": (_I, [_V, C.POINTER(NarutoTrainStep), _I, _I, C.POINTER(_U32)]),
    "naruto_debug_render_plan": (_I, [_V, _U32, _U32, _I, _I, C.POINTER(_U32)]),
    "naruto_render_fwd": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoRender), _V]),
    "naruto_train_backward": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), C.POINTER(NarutoGrads), _U32,
                                   C.POINTER(NarutoFusedAdam), _V]),
    "naruto_track_workspace": (C.c_size_t, [_V, _U32, _U32]),
    "naruto_track_draw": (_I, [C.POINTER(NarutoTrackStep), C.POINTER(NarutoTrainStep), _V]),
    "naruto_track_rays": (_I, [C.POINTER(NarutoTrackStep), C.POINTER(NarutoTrainStep), _V]),
    "naruto_track_backward": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), C.POINTER(NarutoTrackStep), _V]),
    "naruto_ba_poses_workspace": (C.c_size_t, [_V, _U32, _U32]),
    "naruto_ba_poses_init": (_I, [C.POINTER(NarutoBAPoses), _V]),
    "naruto_train_backward_poses": (_I, [_V, C.POINTER(NarutoParams), C.POINTER(NarutoTrainStep), C.POINTER(NarutoGrads), _U32,
                                         C.POINTER(NarutoFusedAdam), C.POINTER(NarutoBAPoses), _V]),
    "naruto_debug_ba_poses_check": (_I, [C.POINTER(NarutoBAPoses), _U32]),
    "naruto_debug_ba_poses_fields": (_I, [C.POINTER(NarutoBAPoses), C.POINTER(_U64)]),
    "naruto_debug_pose_adam": (_I, [C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), C.POINTER(_F), C.c_int32, _F, _F, _F, _F, _F]),
    "naruto_debug_ba_pose_sums": (_I, [_U32, _V, _U32, _V, _U32, _U32, _V, _V, _V, _V, _V, _V]),
    "naruto_debug_rodrigues": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "naruto_compact_active": (_I, [_U32, _U32, _V, _V, _V, _V, _V]),
    "naruto_composite_fwd": (_I, [_V, _U32, _U32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "naruto_composite_bwd": (_I, [_V, _U32, _U32, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _I, _V]),
    "naruto_loss_workspace": (C.c_size_t, [_U32]),
    "naruto_loss_sums": (_I, [_V, _U32, _U32, _V, _V, _V, _V, _V, _V, _V, _F, _F, _V, _V, _V, _V]),
    "naruto_loss_finalize": (_I, [_V, _U64, _U32, _V, _V]),
    "naruto_loss_bwd": (_I, [_V, _U32, _U32, _V, _V, _V, _V, _F, _F, _V, _U64, _V, _V, _V, _V]),
    "naruto_adam_step": (_I, [_V, _V, _V, _V, _U64, _F, _F, _F, _F, _F, _U32, _V, _V]),
    "naruto_debug_mfma_layout": (_I, [_V, _V, _V, _V]),
    "naruto_debug_permlane_swap": (_I, [_V, _V, _V, _V]),
    "naruto_debug_mfma_bf16_layout": (_I, [_V, _V, _V, _V]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: the HIP extension has not been built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). There is no fallback path.")
        # The device pointers and streams handed to the library are PyTorch's, so both must talk to ONE HIP runtime: the
        # one PyTorch-ROCm brings along.  Loaded first, libnaruto_hip.so would pull in /opt/rocm's libamdhip64 and the
        # process would end up with two runtimes (the second one reports "no ROCm-capable device").  Import torch first.
        import torch  # noqa: F401
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


class NarutoError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().naruto_last_error().decode("utf-8", "replace")
        raise NarutoError(f"{what or 'libnaruto_hip'} failed ({rc}): {msg}")


def workspace(n_bytes: int, device, dtype=None, zero: bool = False):
    """The one place a ``naruto_*_workspace()`` byte count becomes a tensor: ``ceil(n_bytes / itemsize)`` elements of ``dtype`` (float32 unless given)."""
    import torch
    dtype = dtype or torch.float32
    return (torch.zeros if zero else torch.empty)(-(-int(n_bytes) // dtype.itemsize), dtype=dtype, device=device)


def kernel_resources(lib_path: str = None):
    """Per kernel of the device code object embedded in the built library: the AMDGPU metadata notes the loader reads
    (``.vgpr_count``, ``.agpr_count``, ``.vgpr_spill_count``, ``.sgpr_spill_count``, ``.private_segment_fixed_size`` = scratch bytes per
    lane, ``.group_segment_fixed_size`` = static LDS).  Uses the ROCm LLVM tools (llvm-objcopy, clang-offload-bundler, llvm-readelf);
    returns {demangled-ish kernel name: {field: int}}.  tests/test_host.py holds the hot kernels to zero scratch with it."""
    import re
    import tempfile
    llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
    lib_path = lib_path or LIB_PATH
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib_path], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "agpr_count":                      # first field of a kernel's record (fields are sorted by name)
            cur = {"agpr_count": int(val)}
        elif cur is not None and key == "name":
            name = re.sub(r"^_ZN6naruto\d+", "", val)
            m2 = re.match(r"(\w+?)(?:I((?:L[bi]\d+E)+)E)?E", name)          # Itanium: name [I <Lb0E | Li128E ...> E] E <signature>
            if m2:
                name = m2.group(1)
                if m2.group(2):
                    args = re.findall(r"L([bi])(\d+)E", m2.group(2))
                    name += "<" + ",".join(("true" if v == "1" else "false") if k == "b" else v for k, v in args) + ">"
            out[name] = cur
        elif cur is not None and key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "sgpr_count", "private_segment_fixed_size",
                                         "group_segment_fixed_size"):
            cur[key] = int(val)
    return out
