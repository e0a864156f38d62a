"""ctypes binding of libdrfe.so (include/drfe.h) — the only way Python reaches the HIP kernels.

There is NO CPU fallback: if the shared library is missing or no HIP device is present the import /
context creation raises.  PyTorch is used by callers only for device buffers and streams; nothing
here depends on it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DRFE_LIB") or os.path.join(_HERE, "csrc", "libdrfe.so")   # DRFE_LIB: variant builds (experiments)

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
MAPPOINT_DTYPE = np.dtype([("valid", "u1"), ("obs_positive", "u1"), ("pad", "u1", (2,)), ("world", "<f4", (3,)),
                           ("desc", "u1", (32,))])
TRACKED_DTYPE = np.dtype([("track_in_view", "u1"), ("bad", "u1"), ("obs_positive", "u1"), ("pad", "u1"),
                          ("level", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"),
                          ("view_cos", "<f4"), ("desc", "u1", (32,))])

STAGES = ("pyramid", "fast", "quadtree", "blur", "desc", "glue", "match", "fast_b")

# every symbol include/drfe.h declares (tests check the library exports all of them)
SYMBOLS = (
    "drfe_create", "drfe_destroy", "drfe_last_error", "drfe_version", "drfe_orb_scale_tables",
    "drfe_orb_max_keypoints", "drfe_orb_extract", "drfe_orb_extract_batch", "drfe_orb_download", "drfe_orb_counts",
    "drfe_orb_pyramid_level", "drfe_orb_blurred_level", "drfe_orb_candidates", "drfe_frame_stereo_grid_batch",
    "drfe_orb_configure_level0", "drfe_orb_level0_in_place", "drfe_orb_quadtree_plan",
    "drfe_fuse_search", "drfe_fuse_search_sim3", "drfe_search_by_sim3", "drfe_search_by_projection_kf", "drfe_search_by_projection_reloc", "drfe_lsd_fuse_search", "drfe_frame_is_in_frustum", "drfe_frame_is_in_frustum_lines", "drfe_frame_set_distortion", "drfe_frame_image_bounds", "drfe_frame_download_keys_un",
    "drfe_frame_download_stereo", "drfe_frame_download_grid", "drfe_match_consecutive_batch", "drfe_match_download",
    "drfe_search_by_projection_last", "drfe_search_by_projection_map", "drfe_match_bf_knn", "drfe_profile_enable",
    "drfe_profile_stage_ms", "drfe_stream_sync", "drfe_planes_ahc", "drfe_planes_ahc_batch", "drfe_planes_ahc_blocks",
    "drfe_match_orb_points", "drfe_planes_cape", "drfe_voc_upload", "drfe_bow_transform_batch", "drfe_bow_download",
    "drfe_search_by_bow", "drfe_search_by_bow_kf", "drfe_search_for_triangulation", "drfe_lsd_extract", "drfe_lsd_extract_batch", "drfe_lsd_stages", "drfe_lines_is_good", "drfe_lsd_search_by_descriptor", "drfe_lsd_search_for_triangulation", "drfe_lsd_search_by_projection_last",
    "drfe_lsd_search_by_projection_map", "drfe_plane_voxel_grid", "drfe_plane_refit", "drfe_planes_ahc_postprocess",
    "drfe_planes_cape_postprocess", "drfe_surface_normals", "drfe_surface_normals_batch", "drfe_surface_normals_download", "drfe_batch_download_async", "drfe_orb_fast_partition", "drfe_orb_fast_cells", "drfe_lsd_segments_host", "drfe_orb_keypoint_pixels_async", "drfe_gather_keypoint_depth",
    "drfe_frame_stereo_grid_batch_kpdepth", "drfe_planes_ahc_post_batch", "drfe_planes_ahc_from_blocks", "drfe_debug_ahc_trials", "drfe_debug_order_sort", "drfe_debug_order_sort_heap_max", "drfe_debug_device_voxel_grid", "drfe_debug_plane_refit", "drfe_search_for_initialization", "drfe_lsd_fuse_search_sim3", "drfe_lsd_search_by_projection_kf",
    "drfe_lsd_search_by_sim3", "drfe_frame_submit", "drfe_frame_collect", "drfe_pipeline_create", "drfe_pipeline_destroy",
    "drfe_pipeline_depth", "drfe_pipeline_context", "drfe_pipeline_last_error", "drfe_pipeline_submit", "drfe_pipeline_sync",
    "drfe_lsd_configure", "drfe_lsd_configure_rect", "drfe_shard_unique_id", "drfe_shard_create", "drfe_shard_destroy", "drfe_shard_broadcast", "drfe_shard_reduce_report", "drfe_shard_sequences_of_rank", "drfe_shard_last_error", "drfe_planes_configure_cape", "drfe_planes_cape_stats", "drfe_lsd_configure_nfa", "drfe_lsd_stats", "drfe_lsd_segments_host_mode", "drfe_debug_cr_sincos", "drfe_debug_device_order_sort", "drfe_debug_device_order_sort_depth", "drfe_batch_status_async", "drfe_batch_check", "drfe_frame_submit_tracked", "drfe_frame_collect_tracked", "drfe_planes_cape_batch", "drfe_planes_configure", "drfe_planes_configure_extractor", "drfe_planes_ahc_stats", "drfe_planes_configure_refit", "drfe_planes_refit_stats", "drfe_frame_load", "drfe_bow_transform_slot", "drfe_long_kernel_clock", "drfe_long_kernel_ms",
    "drfe_manhattan_track_host", "drfe_manhattan_track_batch", "drfe_manhattan_download", "drfe_debug_manhattan_math",
    "drfe_plane_match_host", "drfe_plane_flag_points_host", "drfe_plane_match_status_host", "drfe_plane_map_upload",
    "drfe_plane_match_batch", "drfe_plane_match_download", "drfe_plane_flags_download",
    "drfe_map_plane_update_host", "drfe_map_plane_rebuild_host", "drfe_plane_map_update_batch", "drfe_plane_map_rebuild_batch",
    "drfe_plane_map_edit", "drfe_plane_map_cloud_download", "drfe_plane_map_update_stats",
    "drfe_plane_map_cull_host", "drfe_plane_map_cull_batch", "drfe_plane_map_cull_limits", "drfe_plane_map_cull_stats",
    "drfe_map_point_upkeep_host", "drfe_map_line_upkeep_host", "drfe_map_point_upkeep_batch", "drfe_map_line_upkeep_batch",
    "drfe_map_upkeep_stats",
    "drfe_triangulate_points_host", "drfe_triangulate_lines_host", "drfe_triangulate_points_batch", "drfe_triangulate_lines_batch",
    "drfe_triangulate_stats", "drfe_debug_triangulate_math", "drfe_debug_triangulate_math_device",
    "drfe_sim3_ransac_host", "drfe_sim3_ransac_batch", "drfe_sim3_stats", "drfe_debug_sim3_atan2", "drfe_debug_sim3_rand",
    "drfe_debug_sim3_horn", "drfe_debug_sim3_hand_back",
    "drfe_init_ransac_host", "drfe_init_ransac_batch", "drfe_init_stats",
    "drfe_debug_init_cos_keys", "drfe_debug_init_null_vectors", "drfe_debug_init_check_rt",
    "drfe_pnp_ransac_host", "drfe_pnp_ransac_batch", "drfe_pnp_stats", "drfe_debug_pnp_svd", "drfe_debug_pnp_inliers", "drfe_debug_pnp_inliers_device",
    "drfe_lines_is_good_batch", "drfe_line3d_chunk_frames", "drfe_line3d_stats",
    "drfe_pose_opt_host", "drfe_pose_opt_batch", "drfe_pose_opt_stats", "drfe_debug_cr_cube", "drfe_debug_pose_opt_ldlt",
    "drfe_debug_pose_opt_hand_back", "drfe_debug_pose_opt_plane_error",
    "drfe_trans_opt_host", "drfe_trans_opt_batch", "drfe_trans_opt_stats", "drfe_debug_trans_opt_hand_back",
    "drfe_debug_trans_opt_plane_error",
    "drfe_sim3_opt_host", "drfe_sim3_opt_batch", "drfe_sim3_opt_stats", "drfe_debug_sim3_opt_ldlt", "drfe_debug_sim3_opt_step",
    "drfe_debug_sim3_opt_hand_back",
    "drfe_kfdb_create", "drfe_kfdb_destroy", "drfe_kfdb_last_error", "drfe_kfdb_put", "drfe_kfdb_add", "drfe_kfdb_erase",
    "drfe_kfdb_clear", "drfe_kfdb_remove", "drfe_kfdb_set_neighbours", "drfe_kfdb_size", "drfe_kfdb_loop_queries_host",
    "drfe_kfdb_loop_queries_device", "drfe_kfdb_loop_queries_batch", "drfe_kfdb_reloc_queries_host",
    "drfe_kfdb_reloc_queries_device", "drfe_kfdb_reloc_queries_batch", "drfe_kfdb_score", "drfe_kfdb_stats",
    "drfe_lmap_create", "drfe_lmap_destroy", "drfe_lmap_last_error", "drfe_lmap_configure", "drfe_lmap_limits",
    "drfe_lmap_set_keyframes", "drfe_lmap_set_points", "drfe_lmap_set_lines", "drfe_lmap_set_bad", "drfe_lmap_remove",
    "drfe_lmap_size", "drfe_lmap_update_host", "drfe_lmap_update_device", "drfe_lmap_update_batch", "drfe_lmap_stats",
    "drfe_lmap_set_connections", "drfe_lmap_get_connections", "drfe_lmap_connect_host", "drfe_lmap_connect_device",
    "drfe_lmap_connect_batch", "drfe_lmap_connect_limits", "drfe_lmap_connect_stats",
    "drfe_lmap_set_scales", "drfe_lmap_get_scales", "drfe_lmap_set_poses", "drfe_lmap_get_poses",
    "drfe_lmap_set_point_geometry", "drfe_lmap_get_point_geometry", "drfe_lmap_correct_host", "drfe_lmap_correct_device",
    "drfe_lmap_correct_batch", "drfe_lmap_correct_limits", "drfe_lmap_correct_scratch", "drfe_lmap_correct_stats",
    "drfe_lmap_set_cull_attributes", "drfe_lmap_get_cull_attributes", "drfe_lmap_cull_host", "drfe_lmap_cull_device",
    "drfe_lmap_cull_batch", "drfe_lmap_cull_limits", "drfe_lmap_cull_scratch", "drfe_lmap_cull_stats", "drfe_lmap_upload_bytes",
    "drfe_lmap_set_gba_keyframes", "drfe_lmap_set_gba_points", "drfe_lmap_get_gba_keyframes", "drfe_lmap_get_gba_points",
    "drfe_lmap_gba_host", "drfe_lmap_gba_device", "drfe_lmap_gba_batch", "drfe_lmap_gba_limits", "drfe_lmap_gba_scratch",
    "drfe_lmap_gba_stats",
    "drfe_lmap_set_recent_attributes", "drfe_lmap_get_recent_attributes", "drfe_lmap_recent_increase", "drfe_lmap_recent_cull_host",
    "drfe_lmap_recent_cull_device", "drfe_lmap_recent_cull_batch", "drfe_lmap_recent_cull_limits", "drfe_lmap_recent_cull_scratch",
    "drfe_lmap_recent_cull_stats", "drfe_lmap_recent_upload_bytes",
    "drfe_lmap_fuse_host", "drfe_lmap_fuse_device", "drfe_lmap_fuse_batch", "drfe_lmap_fuse_limits", "drfe_lmap_fuse_scratch",
    "drfe_lmap_fuse_stats", "drfe_lmap_get_replaced", "drfe_lmap_get_match_row", "drfe_lmap_get_observers",
    "drfe_lmap_insert_host", "drfe_lmap_insert_device", "drfe_lmap_insert_batch", "drfe_lmap_insert_limits", "drfe_lmap_insert_scratch",
    "drfe_lmap_insert_stats", "drfe_lmap_create_host", "drfe_lmap_create_device", "drfe_lmap_create_batch",
    "drfe_lmap_create_limits", "drfe_lmap_create_scratch", "drfe_lmap_create_stats",
    "drfe_lmap_set_loop_edges", "drfe_lmap_get_loop_edges", "drfe_lmap_essential_upload_bytes", "drfe_lmap_essential_edges_host",
    "drfe_lmap_essential_edges_device", "drfe_lmap_essential_edges_batch", "drfe_lmap_essential_commit_host",
    "drfe_lmap_essential_commit_device", "drfe_lmap_essential_commit_batch", "drfe_lmap_essential_limits",
    "drfe_lmap_essential_scratch", "drfe_lmap_essential_stats",
)

FAST_CELL_DTYPE = np.dtype([(n, "<i4") for n in ("level", "x0", "y0", "ww", "wh", "offX", "offY", "cellIdx", "ncp", "rpl", "nrb",
                                                  "kernel", "list_cap")])   # drfe_orb_fast_cells, DRFE_FAST_CELL_FIELDS int32
FRUSTUM_POINT_DTYPE = np.dtype([("world", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"),
                                ("max_distance", "<f4")])                            # drfe_frustum_point, 32 B
FRUSTUM_LINE_DTYPE = np.dtype([("world", "<f8", (6,)), ("normal", "<f8", (3,)), ("min_distance", "<f4"),
                               ("max_distance", "<f4")])                             # drfe_frustum_line, 80 B
MAPLINE_DTYPE = np.dtype([("valid", "<i4"), ("octave", "<i4"), ("obs_positive", "<i4"), ("pad", "<i4"),
                          ("world", "<f8", (6,)), ("desc", "u1", (32,))])            # drfe_map_line, 96 B
TRACKED_LINE_DTYPE = np.dtype([("in_view", "<i4"), ("level", "<i4"), ("obs_positive", "<i4"), ("x1", "<f4"),
                               ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("view_cos", "<f4"),
                               ("desc", "u1", (32,))])                                # drfe_tracked_line, 64 B
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("start_point_x", "<f4"), ("start_point_y", "<f4"),
                          ("end_point_x", "<f4"), ("end_point_y", "<f4"), ("s_point_in_octave_x", "<f4"),
                          ("s_point_in_octave_y", "<f4"), ("e_point_in_octave_x", "<f4"), ("e_point_in_octave_y", "<f4"),
                          ("line_length", "<f4"), ("num_of_pixels", "<i4")])

CAPE_PLANE_DTYPE = np.dtype([("normal", "<f8", (3,)), ("mean", "<f8", (3,)), ("d", "<f8"), ("mse", "<f4"),
                             ("score", "<f4"), ("n_points", "<i4"), ("pad", "<i4")])

PLANE_POST_DTYPE = np.dtype([("coef", "<f4", (4,)), ("accepted", "<i4"), ("n_voxels", "<i4")])      # drfe_plane_post, 24 B
SURFACE_NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("camera_position", "<f4", (3,)), ("frame_x", "<i4"),
                                 ("frame_y", "<i4")])                                               # drfe_surface_normal, 32 B

MANHATTAN_CALL_DTYPE = np.dtype([("in_cone", "<i4", (3,)), ("n_selected", "<i4", (3,)), ("threshold", "<i4"),
                                 ("deficient", "<i4"), ("found", "<i4"), ("svd", "<i4"), ("density", "<f4", (3,)),
                                 ("pad", "<i4")])                                           # drfe_manhattan_call, 56 B
MANHATTAN_MAX_CALLS = 5
MANHATTAN_INLINE_BIT = 0x8000
MANHATTAN_INFO_DTYPE = np.dtype([("n_calls", "<i4"), ("pad", "<i4"),
                                 ("call", MANHATTAN_CALL_DTYPE, (MANHATTAN_MAX_CALLS,))])   # drfe_manhattan_info, 288 B

# drfe_plane_match_params (dTh, aTh, verTh, parTh): PlaneMatcher's constructor defaults, as the float arguments receive them
PLANE_MATCH_DEFAULTS = np.array([0.1, 0.86, 0.08716, 0.9962], np.float32)

PLANE_DTYPE = np.dtype([("normal", "<f8", (3,)), ("center", "<f8", (3,)), ("mse", "<f8"), ("curvature", "<f8"),
                        ("n_points", "<i4"), ("rid", "<i4")])


class DrfeError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32),
                ("max_batch", C.c_int32), ("nfeatures", C.c_int32), ("scale_factor", C.c_float),
                ("nlevels", C.c_int32), ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32)]


class UpkeepKeyframes(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_levels", C.c_int32), ("center", C.c_void_p), ("bad", C.c_void_p),
                ("scale_factors", C.c_void_p)]                                       # drfe_upkeep_keyframes


class UpkeepItems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("bad", C.c_void_p), ("obs_offsets", C.c_void_p), ("obs_kf", C.c_void_p),
                ("obs_desc", C.c_void_p), ("world", C.c_void_p), ("ref_kf", C.c_void_p), ("ref_level", C.c_void_p)]   # drfe_upkeep_items


class UpkeepOut(C.Structure):
    _fields_ = [("best_obs", C.c_void_p), ("desc", C.c_void_p), ("normal", C.c_void_p), ("max_distance", C.c_void_p),
                ("min_distance", C.c_void_p), ("status", C.c_void_p), ("frustum", C.c_void_p)]              # drfe_upkeep_out


UPKEEP_DESCRIPTOR, UPKEEP_NORMAL = 1, 2
UPKEEP_DEVICE_ROWS = 2048
UPKEEP_STATS = ("calls", "items", "desc_b4", "desc_b16", "desc_b64", "desc_wg", "desc_host", "normals")

TRI_KF_DTYPE = np.dtype([("Tcw", np.float32, 12), ("Twc", np.float32, 12), ("Ow", np.float32, 3), ("fx", np.float32),
                         ("fy", np.float32), ("cx", np.float32), ("cy", np.float32), ("invfx", np.float32), ("invfy", np.float32),
                         ("mb", np.float32), ("mbf", np.float32), ("scale_factor", np.float32)])   # drfe_tri_keyframe


class TriKeyframes(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_levels", C.c_int32), ("kf", C.c_void_p), ("scale_factors", C.c_void_p),
                ("level_sigma2", C.c_void_p)]                                        # drfe_tri_keyframes


class TriKeypoints(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("un", C.c_void_p), ("raw", C.c_void_p), ("octave", C.c_void_p),
                ("u_right", C.c_void_p), ("depth", C.c_void_p)]                      # drfe_tri_keypoints


class TriKeylines(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("ends", C.c_void_p), ("octave", C.c_void_p), ("depth", C.c_void_p),
                ("lines3d", C.c_void_p)]                                             # drfe_tri_keylines


class TriPairs(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("kf1", C.c_void_p), ("kf2", C.c_void_p), ("match_offsets", C.c_void_p),
                ("matches", C.c_void_p)]                                             # drfe_tri_pairs


class TriOut(C.Structure):
    _fields_ = [("status", C.c_void_p), ("branch", C.c_void_p), ("x3d", C.c_void_p), ("pair_skipped", C.c_void_p),
                ("accepted", C.c_void_p)]                                            # drfe_tri_out


# status codes (DRFE_TRI_*): points and lines share 0-2; the flag marks a line match whose idx2 is past KF1's key lines
TRI_ACCEPTED, TRI_BASELINE, TRI_NO_PARALLAX = 0, 1, 2
TRI_POINT_CODES = ("accepted", "baseline", "no_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "dist", "scale")
TRI_LINE_CODES = ("accepted", "baseline", "no_stereo", "z_sp1", "z_ep1", "z_sp2", "z_ep2", "reproj_sp1", "reproj_ep1",
                  "reproj_sp2", "reproj_ep2", "dist", "scale")
TRI_IDX2_PAST_KF1 = 0x80
TRI_BRANCH_NONE, TRI_BRANCH_SVD, TRI_BRANCH_STEREO1, TRI_BRANCH_STEREO2 = 0, 1, 2, 3
TRI_STATS = ("calls", "pairs", "pairs_skipped", "matches", "svd", "stereo1", "stereo2", "accepted")


class Sim3Problems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("Tcw1", C.c_void_p), ("Tcw2", C.c_void_p), ("K1", C.c_void_p),
                ("K2", C.c_void_p), ("fix_scale", C.c_void_p), ("probability", C.c_void_p), ("min_inliers", C.c_void_p),
                ("max_iterations", C.c_void_p), ("seed", C.c_void_p), ("offsets", C.c_void_p), ("Xw1", C.c_void_p),
                ("Xw2", C.c_void_p), ("sigma2_1", C.c_void_p), ("sigma2_2", C.c_void_p)]    # drfe_sim3_problems


class PnpProblems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "K", "probability", "min_inliers", "max_iterations", "epsilon", "th2", "tail", "seed", "offsets", "p2d", "Xw",
        "sigma2")]                                                                   # drfe_pnp_problems


PNP_OUT_FIELDS = ("iterations", "min_inliers", "hypotheses", "refines", "sample", "R", "t", "inliers", "mask", "best", "returns",
                  "refined_R", "refined_t", "refined_inliers", "refined_mask")


class PnpOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in PNP_OUT_FIELDS]                             # drfe_pnp_out


class PoseOptProblems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "Tcw", "K", "bf", "b_struct", "point_offsets", "obs", "u_right", "inv_sigma2", "Xw", "line_offsets", "line_fn",
        "line_ends", "plane_offsets", "plane_meas", "plane_world", "plane_mask")] + [
        ("plane_settings", C.c_double * 7)]                                          # drfe_pose_opt_problems


POSE_OPT_OUT_FIELDS = ("Tcw", "returns", "rounds", "iterations", "trials", "diag", "point_outlier", "line_outlier", "plane_outlier",
                       "par_plane_outlier", "ver_plane_outlier")
POSE_OPT_DIAG = ("rejected", "last_rejected", "nbad_stops", "small_theta", "big_theta", "empty_rounds")
POSE_OPT_MAX_FRAMES, POSE_OPT_MAX_POINTS, POSE_OPT_MAX_LINES, POSE_OPT_MAX_PLANES = 4096, 8192, 1024, 64
POSE_OPT_PLANE_MATCHED, POSE_OPT_PLANE_PARALLEL, POSE_OPT_PLANE_VERTICAL = 1, 2, 4
POSEOPT_DEVICE_FROM = 64
POSE_OPT_STATS = ("calls", "frames", "point_edges", "line_plane_edges", "iterations", "trials", "handed_back", "frames_too_few")


class PoseOptOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in POSE_OPT_OUT_FIELDS]                        # drfe_pose_opt_out


SIM3_OPT_IN_FIELDS = ("S12", "K1", "K2", "R1w", "t1w", "R2w", "t2w", "th2", "fix_scale", "match_offsets", "index", "P3D1w", "P3D2w",
                      "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")
SIM3_OPT_OUT_FIELDS = ("S12", "T12", "Scw", "returns", "n_bad", "iterations", "trials", "diag", "outlier")
SIM3_OPT_DIAG = ("rejected", "last_rejected", "nbad_stops", "small_theta", "big_theta", "early_return", "stale_decided")
SIM3_OPT_MAX_PROBLEMS, SIM3_OPT_MAX_MATCHES = 1024, 8192
SIM3OPT_DEVICE_FROM = 8                              # DRFE_SIM3OPT_DEVICE_FROM
SIM3_OPT_STATS = ("calls", "problems", "matches", "free_scale", "iterations", "trials", "handed_back", "early_returns")


class Sim3OptProblems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in SIM3_OPT_IN_FIELDS]   # drfe_sim3_opt_problems


class Sim3OptOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in SIM3_OPT_OUT_FIELDS]                        # drfe_sim3_opt_out


KFDB_L1_NORM, KFDB_L2_NORM, KFDB_CHI_SQUARE, KFDB_KL, KFDB_BHATTACHARYYA, KFDB_DOT_PRODUCT = range(6)   # DBoW2::ScoringType
KFDB_NEIGHBOURS = 10
KFDB_DEVICE_FROM = 16                                                                # DRFE_KFDB_DEVICE_FROM
KFDB_STATS = ("loop_calls", "loop_queries", "reloc_calls", "reloc_queries", "device_calls", "uploads", "candidates",
              "uninit_reads")
ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_STATE = -1, -2, -3, -4


class KfdbLoopQueries(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "handle", "id", "connected_offsets", "connected", "min_score", "covisible_offsets", "covisible",
        "add_after")]                                                                # drfe_kfdb_loop_queries


class KfdbRelocQueries(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "id", "word_offsets", "word_ids", "values")]                                 # drfe_kfdb_reloc_queries


class KfdbOut(C.Structure):
    _fields_ = [("cand_capacity", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "cand_offsets", "candidates", "record", "min_score", "uninit_reads")]        # drfe_kfdb_out


LMAP_NEIGHBOURS = 10
LMAP_KEYFRAME, LMAP_POINT, LMAP_LINE = range(3)                                      # the kinds of drfe_lmap_set_bad / _remove
LMAP_STATS = ("calls", "queries", "device_calls", "uploads", "local_kfs", "local_points", "local_lines", "nulled")
LMAP_LIMITS = ("lds_keyframes", "vote_threads", "gather_entries", "device_from")


class LmapKeyframes(C.Structure):
    _fields_ = [("count", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "handle", "rank", "bad", "parent", "neighbours", "child_offsets", "children", "point_offsets", "points",
        "line_offsets", "lines")]                                                    # drfe_lmap_keyframes


class LmapQueries(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "frame_id", "point_offsets", "points", "line_offsets", "lines", "prev_kf_offsets", "prev_kfs")]   # drfe_lmap_queries


LMAP_OUT_FIELDS = ("kf_offsets", "kfs", "ref_kf", "mp_offsets", "mps", "mp_in_frame", "ml_offsets", "mls", "ml_in_frame",
                   "nulled_offsets", "nulled", "record")


class LmapOut(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kf_capacity", "mp_capacity", "ml_capacity", "nulled_capacity")] + [
        (k, C.c_void_p) for k in LMAP_OUT_FIELDS]                                    # drfe_lmap_out


LMAP_CONNECT_TH = 15
LMAP_CONNECT_STATS = ("calls", "keyframes", "device_calls", "counter_entries", "listed", "touched", "first_connections",
                      "empty_counters")
LMAP_CONNECT_LIMITS = ("threshold", "device_from", "sort_tile", "row_groups")
CONN_WEIGHTS, CONN_ORDERED, CONN_PARENT = 1, 2, 4                                    # the bits of drfe_lmap_connect_out.flags


class LmapConnections(C.Structure):
    _fields_ = [("count", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "handle", "first_connection", "weight_offsets", "weight_kfs", "weight_w", "ordered_offsets", "ordered_kfs",
        "ordered_w")]                                                                # drfe_lmap_connections


LMAP_CONN_ROWS_FIELDS = ("weight_offsets", "weight_kfs", "weight_w", "ordered_offsets", "ordered_kfs", "ordered_w", "parent",
                         "first_connection")


class LmapConnRows(C.Structure):
    _fields_ = [("weights_capacity", C.c_int32), ("ordered_capacity", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_CONN_ROWS_FIELDS]                              # drfe_lmap_conn_rows


class LmapConnectOut(C.Structure):
    _fields_ = [("counter_capacity", C.c_int32), ("touched_capacity", C.c_int32)] + [(k, C.c_void_p) for k in (
        "counter_offsets", "counter_kfs", "counter_votes", "record", "new_parent", "n_touched", "touched")] + [
        ("rows", LmapConnRows), ("flags", C.c_void_p)]                               # drfe_lmap_connect_out


LMAP_CORRECT_STATS = ("calls", "keyframes", "device_calls", "moved", "moved_without_obs", "entries_walked", "device_chunks",
                      "geometry_uploads")
LMAP_CORRECT_LIMITS = ("claim_tile", "device_from", "entry_bytes", "threads")


class LmapPointGeometry(C.Structure):
    _fields_ = [("count", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "handle", "world", "ref_kf", "ref_level", "corrected_by", "corrected_ref")]  # drfe_lmap_point_geometry


LMAP_CORRECT_OUT_FIELDS = ("walk_pos", "corrected", "non_corrected", "Tiw", "n_points", "points", "claimed_by", "world", "normal",
                           "max_distance", "min_distance", "status")


class LmapCorrectOut(C.Structure):
    _fields_ = [("points_capacity", C.c_int32), ("pad", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_CORRECT_OUT_FIELDS]                            # drfe_lmap_correct_out


LMAP_GBA_STATS = ("calls", "device_calls", "visited", "composed", "deepest_chain", "kind_pos", "kind_ref", "skipped_ref")
LMAP_GBA_LIMITS = ("threads", "device_from", "depth_limit", "point_bytes", "fixed_bytes", "wavefront")
GBA_POINT_POS, GBA_POINT_REF = 1, 2                                                  # drfe_lmap_gba_out.kind
LMAP_GBA_OUT_FIELDS = ("n_keyframes", "keyframes", "Tcw", "TcwBef", "composed", "n_points", "points", "world", "kind")


class LmapGbaOut(C.Structure):
    _fields_ = [("keyframes_capacity", C.c_int32), ("points_capacity", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_GBA_OUT_FIELDS]                                # drfe_lmap_gba_out


LMAP_CULL_STATS = ("calls", "keyframes", "device_calls", "culled", "deferred", "points_bad", "observers_walked", "empty_begin")
LMAP_CULL_LIMITS = ("record_tile", "device_from", "entry_bytes", "walk_threads")
CULL_NOT_ERASE, CULL_ORIGIN, CULL_TO_BE_ERASED = 1, 2, 4                             # the bits of a key frame's flags byte
CULL_KEPT, CULL_CULLED, CULL_DEFERRED, CULL_SKIPPED_ORIGIN = 0, 1, 2, 3              # record[:, 3]
# the bits of drfe_lmap_cull_out.flags after CONN_WEIGHTS, CONN_ORDERED, CONN_PARENT
CULL_CHILDREN, CULL_NULLED, CULL_WENT_BAD = 8, 16, 32
LMAP_CULL_ATTR_FIELDS = ("kf_handle", "th_depth", "kf_flags", "row_offsets", "octave", "depth", "stereo", "point_handle", "n_obs",
                         "obs_offsets", "obs_index")


class LmapCullAttributes(C.Structure):
    _fields_ = [("n_kfs", C.c_int32), ("n_points", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_CULL_ATTR_FIELDS]                              # drfe_lmap_cull_attributes


class LmapCullAttributesOut(C.Structure):
    _fields_ = [("n_kfs", C.c_int32), ("n_points", C.c_int32), ("row_capacity", C.c_int32), ("obs_capacity", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_CULL_ATTR_FIELDS]                              # drfe_lmap_cull_attributes_out


class LmapCullOut(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("touched_capacity", "children_capacity", "nulled_capacity", "points_capacity",
                                         "obs_capacity", "pad")] + [(k, C.c_void_p) for k in (
        "record", "Tcp", "has_Tcp", "n_culled", "culled", "n_touched", "touched")] + [("rows", LmapConnRows)] + [
        (k, C.c_void_p) for k in ("flags", "children_offsets", "children", "nulled_offsets", "nulled", "n_points", "points",
                                  "point_n_obs", "point_ref", "point_bad", "obs_offsets", "obs", "obs_index")]   # drfe_lmap_cull_out


LMAP_RECENT_STATS = ("calls", "entries", "device_calls", "culled_ratio", "culled_observations", "aged_out", "dropped_bad", "nulled")
LMAP_RECENT_LIMITS = ("entry_tile", "erase_tile", "entry_bytes", "wavefront", "max_entries", "device_from")
RECENT_KEPT, RECENT_WAS_BAD, RECENT_RATIO, RECENT_OBSERVATIONS, RECENT_AGED = range(5)   # drfe_lmap_recent_list.action
LMAP_RECENT_ATTR_FIELDS = ("point_handle", "point_found", "point_visible", "point_first_kf", "line_handle", "line_found",
                           "line_visible", "line_first_kf", "line_n_obs", "line_obs_offsets", "line_obs", "line_obs_index")


class LmapRecentAttributes(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_lines", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_RECENT_ATTR_FIELDS]                            # drfe_lmap_recent_attributes


class LmapRecentAttributesOut(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_lines", C.c_int32), ("line_obs_capacity", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_RECENT_ATTR_FIELDS]                            # drfe_lmap_recent_attributes_out


class LmapRecentList(C.Structure):
    _fields_ = [("n", C.c_int32), ("handles", C.c_void_p), ("erased_capacity", C.c_int32)] + [(k, C.c_void_p) for k in (
        "action", "n_kept", "kept", "n_culled", "culled", "erased_offsets", "erased_kf", "erased_index")]   # drfe_lmap_recent_list


LMAP_FUSE_STATS = ("calls", "candidates", "device_calls", "added", "replaced", "moved", "erased", "handed_back")
LMAP_FUSE_LIMITS = ("tile", "wavefront", "log_entries", "record_entries", "max_kfs", "tile_bytes", "max_candidates", "device_from")
FUSE_NEIGHBOURS, FUSE_LOOP, FUSE_MATCHED = range(3)                                   # drfe_lmap_fuse_step.form
(FUSE_NONE, FUSE_SKIPPED, FUSE_ADDED, FUSE_ROW_ONLY, FUSE_OCCUPANT_BAD, FUSE_CANDIDATE_REPLACED, FUSE_OCCUPANT_REPLACED, FUSE_SELF,
 FUSE_RECORDED) = range(9)                                                            # drfe_lmap_fuse_step.action


class LmapFuseStep(C.Structure):
    _fields_ = [("keyframe", C.c_int32), ("kind", C.c_int32), ("form", C.c_int32), ("n", C.c_int32)] + [(k, C.c_void_p) for k in (
        "candidates", "best_idx", "action", "n_fused", "replace")]                   # drfe_lmap_fuse_step


class LmapFuseCall(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("steps", C.c_void_p), ("replaced_capacity", C.c_int32), ("record_capacity", C.c_int32),
                ("touched_capacity", C.c_int32)] + [(k, C.c_void_p) for k in (
        "n_replaced", "replaced_kind", "loser", "winner", "record_offsets", "record_kf", "record_index", "record_moved",
        "n_touched", "touched_points", "touched_lines")]                             # drfe_lmap_fuse_call


LMAP_INSERT_STATS = ("calls", "keyframes", "device_calls", "points_added", "lines_added", "recent_points", "recent_lines", "device_chunks")
LMAP_INSERT_LIMITS = ("tile", "wavefront", "claim_bytes", "normal_groups", "threads", "max_keyframes", "device_from", "reserved")
INSERT_NULL, INSERT_BAD, INSERT_RECENT, INSERT_ADDED = range(4)                       # drfe_lmap_insert_call's action bytes
LMAP_INSERT_CALL_FIELDS = ("point_offsets", "point_action", "line_offsets", "line_action", "n_added", "added_points", "added_point_kf",
                           "added_point_index", "normal", "max_distance", "min_distance", "status", "added_lines", "added_line_kf",
                           "added_line_index", "n_recent", "recent_points", "recent_lines")


class LmapInsertCall(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32), ("handles", C.c_void_p), ("action_capacity", C.c_int32 * 2),
                ("added_capacity", C.c_int32 * 2), ("recent_capacity", C.c_int32 * 2)] + [
        (k, C.c_void_p) for k in LMAP_INSERT_CALL_FIELDS]                           # drfe_lmap_insert_call


LMAP_ESSENTIAL_STATS = ("edges_calls", "commit_calls", "device_calls", "vertices", "edges", "points_moved", "points_identity",
                        "prefixes_emptied")
LMAP_ESSENTIAL_LIMITS = ("threads", "wavefront", "edges_device_from", "commit_device_from", "point_bytes", "kf_bytes", "edge_bytes",
                         "vertex_bytes")
ESSENTIAL_MIN_FEAT = 100                                                             # DRFE_LMAP_ESSENTIAL_MIN_FEAT
ESSENTIAL_LOOP_CONNECTION, ESSENTIAL_SPANNING_TREE, ESSENTIAL_LOOP_EDGE, ESSENTIAL_COVISIBILITY = 0, 1, 2, 3   # ..._edges_call.kind
LMAP_ESSENTIAL_EDGES_IN = ("sim3_handles", "corrected", "non_corrected", "lc_handles", "lc_offsets", "lc_kfs")
LMAP_ESSENTIAL_EDGES_OUT = ("n_vertices", "vertices", "Scw", "fixed", "n_edges", "from", "to", "measurement", "kind")
LMAP_ESSENTIAL_COMMIT_OUT = ("Tiw", "Swc", "n_points", "points", "ref", "world", "normal", "max_distance", "min_distance", "status")


class LmapEssentialEdgesCall(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("loop_kf", "cur_kf", "n_sim3", "n_lc")] + [(k, C.c_void_p) for k in LMAP_ESSENTIAL_EDGES_IN] +
                [("vertices_capacity", C.c_int32), ("edges_capacity", C.c_int32)] +
                [(k, C.c_void_p) for k in LMAP_ESSENTIAL_EDGES_OUT])                 # drfe_lmap_essential_edges_call


class LmapEssentialCommitCall(C.Structure):
    _fields_ = ([("cur_kf", C.c_int32), ("n", C.c_int32)] + [(k, C.c_void_p) for k in ("handles", "Scw", "optimised")] +
                [("points_capacity", C.c_int32), ("pad", C.c_int32)] +
                [(k, C.c_void_p) for k in LMAP_ESSENTIAL_COMMIT_OUT])                # drfe_lmap_essential_commit_call


LMAP_CREATE_STATS = ("calls", "device_calls", "points_created", "lines_created", "displaced", "stale_calls", "relayouts", "device_chunks")
LMAP_CREATE_LIMITS = ("tile", "wavefront", "claim_bytes", "item_bytes", "threads", "reserved0", "device_from", "reserved1")
LMAP_CREATE_IN_FIELDS = ("point_handle", "point_n_obs", "point_obs_kf", "point_obs_index", "point_ref_kf", "point_first_kf", "point_world",
                         "line_handle", "line_n_obs", "line_obs_kf", "line_obs_index", "line_ref_kf", "line_first_kf")
LMAP_CREATE_OUT_FIELDS = ("point_displaced", "line_displaced", "normal", "max_distance", "min_distance", "status")


class LmapCreateCall(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_lines", C.c_int32)] + [(k, C.c_void_p) for k in LMAP_CREATE_IN_FIELDS] + [
        ("displaced_capacity", C.c_int32 * 2), ("record_capacity", C.c_int32), ("pad", C.c_int32)] + [
        (k, C.c_void_p) for k in LMAP_CREATE_OUT_FIELDS]                            # drfe_lmap_create_call


class InitProblems(C.Structure):
    _fields_ = [("n", C.c_int32), ("pad", C.c_int32)] + [(k, C.c_void_p) for k in (
        "K", "sigma", "max_iterations", "seed", "key1_offsets", "key2_offsets", "keys1", "keys2",
        "matches12")]                                                                # drfe_init_problems


INIT_OUT_FIELDS = ("N", "iterations", "hypotheses", "SH", "SF", "RH", "branch", "motions", "ok", "flags", "R21", "t21", "vP3D",
                   "vbTriangulated", "sample", "H21", "F21", "score_h", "score_f", "best_h", "best_f", "mask_h", "mask_f",
                   "motion_R", "motion_t", "motion_good", "motion_cos", "motion_parallax", "motion_status", "motion_vbGood",
                   "motion_vP3D")
INIT_BRANCH_NONE, INIT_BRANCH_H, INIT_BRANCH_F = 0, 1, 2
INIT_TOO_FEW, INIT_NO_MODEL, INIT_H_DEGENERATE = 1, 2, 4
INIT_MOTION_NAN_COS = 1
INIT_MAX_KEYS, INIT_MAX_ITERATIONS, INIT_MAX_SOLVERS, INIT_MAX_ROWS, INIT_MAX_MASK_WORDS = 4096, 300, 65535, 1 << 20, 1 << 24
INIT_STATS = ("calls", "solvers", "rows", "matches", "branch_h", "branch_f", "ok", "empty")


class InitOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in INIT_OUT_FIELDS]                            # drfe_init_out


class Sim3Out(C.Structure):
    _fields_ = [("iterations", C.c_void_p), ("hypotheses", C.c_void_p), ("sample", C.c_void_p), ("R12", C.c_void_p),
                ("t12", C.c_void_p), ("s12", C.c_void_p), ("T12", C.c_void_p), ("inliers", C.c_void_p), ("returns", C.c_void_p),
                ("best", C.c_void_p), ("mask", C.c_void_p)]                          # drfe_sim3_out


SIM3_MAX_CORR, SIM3_MAX_ITERATIONS = 4096, 300
SIM3_STATS = ("calls", "solvers", "hypotheses", "correspondences", "solvers_lds", "solvers_global", "uncertified", "solvers_empty")
PNP_STATS = ("calls", "solvers", "hypotheses", "correspondences", "refine_jobs", "refine_points", "solvers_global", "solvers_empty")
LINE3D_STATS = ("calls", "frames", "lines", "ransac_lines", "iterations", "coincident_pairs", "verify_rejections", "accepted")
LINE3D_MAX_CAP = 4096


class Line3dFrames(C.Structure):
    _fields_ = [("nframes", C.c_int32), ("cap", C.c_int32), ("lines", C.c_void_p), ("n_lines", C.c_void_p), ("depth", C.c_void_p),
                ("frame_stride", C.c_size_t), ("stride", C.c_size_t), ("w", C.c_int32), ("h", C.c_int32),
                ("depth_on_device", C.c_int32), ("k_as_f64", C.c_int32), ("K", C.c_float * 9), ("cx", C.c_float),
                ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("seeds", C.c_void_p)]   # drfe_line3d_frames


class Line3dOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("depth_line", "lines3d", "n_inliers", "n_good")]              # drfe_line3d_out


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("depth_factor", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float)]


_lib = None


def load() -> C.CDLL:
    """Load libdrfe.so; raises if it was not built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DrfeError(f"{LIB_PATH} not found: build it with `make -C dr_slam_amd/csrc` "
                        "(there is no CPU fallback for the feature path)")
    # One HIP runtime per process: PyTorch ships its own libamdhip64; if libdrfe pulled in the system
    # copy first, a later `import torch` would bring a second runtime that cannot see the device.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.drfe_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.drfe_destroy.argtypes = [vp]
    L.drfe_destroy.restype = None
    L.drfe_last_error.argtypes = [vp]
    L.drfe_last_error.restype = C.c_char_p
    L.drfe_version.restype = C.c_char_p
    L.drfe_orb_scale_tables.argtypes = [vp, vp, vp, vp, vp]
    L.drfe_orb_max_keypoints.argtypes = [vp]
    L.drfe_orb_extract.argtypes = [vp, vp, i32, i32, sz, vp, vp, i32, C.POINTER(i32)]
    L.drfe_orb_extract_batch.argtypes = [vp, vp, sz, sz, i32, i32, i32, vp]
    L.drfe_pipeline_create.argtypes = [C.POINTER(Config), i32, C.POINTER(vp)]
    L.drfe_pipeline_destroy.argtypes = [vp]
    L.drfe_pipeline_destroy.restype = None
    L.drfe_pipeline_depth.argtypes = [vp]
    L.drfe_pipeline_context.argtypes = [vp, i32]
    L.drfe_pipeline_context.restype = vp
    L.drfe_pipeline_last_error.argtypes = [vp]
    L.drfe_pipeline_last_error.restype = C.c_char_p
    L.drfe_pipeline_submit.argtypes = [vp, vp, vp, sz, sz, i32, i32, vp, vp, C.POINTER(Camera), C.c_float, i32, i32, i32]
    L.drfe_pipeline_sync.argtypes = [vp, i32]
    L.drfe_frame_submit.argtypes = [vp, i32, vp, i32, i32, sz, vp, sz, C.POINTER(Camera)]
    L.drfe_frame_collect.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.drfe_frame_submit_tracked.argtypes = [vp, i32, vp, i32, i32, sz, vp, sz, C.POINTER(Camera), i32, vp, vp, vp, vp, i32, f32, i32, i32]
    L.drfe_frame_collect_tracked.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)]
    L.drfe_orb_download.argtypes = [vp, i32, vp, vp, i32, C.POINTER(i32)]
    L.drfe_orb_counts.argtypes = [vp, i32, vp]
    L.drfe_orb_fast_partition.argtypes = [vp, i32, i32, vp, vp]
    L.drfe_orb_fast_cells.argtypes = [vp, i32, i32, vp, i32, vp]
    L.drfe_orb_keypoint_pixels_async.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_gather_keypoint_depth.argtypes = [vp, sz, sz, i32, vp, vp, i32, vp, i32]
    L.drfe_frame_stereo_grid_batch_kpdepth.argtypes = [vp, vp, i32, C.POINTER(Camera), i32, vp]
    L.drfe_batch_download_async.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.drfe_orb_pyramid_level.argtypes = [vp, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.drfe_orb_configure_level0.argtypes = [vp, i32]
    L.drfe_orb_level0_in_place.argtypes = [vp]
    L.drfe_orb_blurred_level.argtypes = [vp, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]
    L.drfe_orb_candidates.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.drfe_frame_stereo_grid_batch.argtypes = [vp, vp, sz, sz, C.POINTER(Camera), i32, vp]
    L.drfe_frame_download_stereo.argtypes = [vp, i32, vp, vp, i32]
    L.drfe_frame_download_grid.argtypes = [vp, i32, vp, vp, i32]
    L.drfe_match_consecutive_batch.argtypes = [vp, vp, vp, C.POINTER(Camera), f32, i32, i32, i32, vp]
    L.drfe_match_download.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.drfe_search_by_projection_last.argtypes = [vp, i32, i32, vp, vp, C.POINTER(Camera), vp, i32, f32, i32, i32,
                                                 vp, vp, i32, C.POINTER(i32)]
    L.drfe_search_by_projection_map.argtypes = [vp, i32, vp, i32, f32, f32, vp, vp, i32, C.POINTER(i32)]
    L.drfe_match_bf_knn.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp]
    L.drfe_match_orb_points.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, C.POINTER(i32)]
    L.drfe_search_by_bow_kf.argtypes = [vp, i32, i32, vp, i32, vp, i32, C.c_float, i32, vp, C.POINTER(i32)]
    L.drfe_search_for_triangulation.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, C.POINTER(i32)]
    L.drfe_planes_ahc_batch.argtypes = [vp, vp, C.c_size_t, i32, i32, C.c_size_t, i32, vp, C.c_float, vp, i32, vp, vp, vp, vp, i32]
    L.drfe_lsd_extract_batch.argtypes = [vp, vp, C.c_size_t, i32, i32, C.c_size_t, i32, i32, vp, vp, vp, i32, vp, vp, i32]
    L.drfe_lines_is_good.argtypes = [vp, i32, vp, i32, i32, C.c_size_t, vp, i32, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_uint32, vp, vp, vp, C.POINTER(i32)]
    L.drfe_lsd_fuse_search.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp]
    L.drfe_lsd_fuse_search_sim3.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, vp, vp]
    L.drfe_lsd_search_by_projection_kf.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, i32, vp, C.POINTER(i32)]
    L.drfe_lsd_search_by_sim3.argtypes = [vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.c_float,
                                          vp, C.POINTER(i32)]
    L.drfe_search_by_projection_reloc.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, C.c_float, i32, i32, vp, C.POINTER(i32)]
    L.drfe_search_for_initialization.argtypes = [vp, i32, i32, vp, i32, i32, C.c_float, i32, vp, C.POINTER(i32)]
    L.drfe_search_by_projection_kf.argtypes = [vp, i32, vp, vp, vp, vp, i32, vp, i32, C.c_float, vp, C.POINTER(i32)]
    L.drfe_search_by_sim3.argtypes = [vp, i32, i32, vp, vp, C.c_float, vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, C.c_float, vp,
                                      C.POINTER(i32)]
    L.drfe_fuse_search_sim3.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, vp]
    L.drfe_fuse_search.argtypes = [vp, i32, vp, vp, vp, vp, i32, C.c_float, vp, vp]
    L.drfe_frame_is_in_frustum.argtypes = [vp, vp, vp, vp, i32, C.c_float, vp]
    L.drfe_frame_is_in_frustum_lines.argtypes = [vp, vp, vp, vp, i32, C.c_float, vp]
    L.drfe_frame_set_distortion.argtypes = [vp, vp, vp, i32]
    L.drfe_frame_image_bounds.argtypes = [vp, vp, i32, i32, i32, vp]
    L.drfe_frame_download_keys_un.argtypes = [vp, i32, vp, i32]
    L.drfe_lsd_search_for_triangulation.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.drfe_lsd_search_by_descriptor.argtypes = [vp, vp, i32, vp, i32, vp, i32, vp, C.POINTER(i32)]
    L.drfe_lsd_search_by_projection_last.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, i32, C.c_float, i32, C.c_float, vp, vp,
                                                     C.POINTER(i32)]
    L.drfe_lsd_search_by_projection_map.argtypes = [vp, vp, i32, vp, vp, i32, C.c_float, C.c_float, vp, vp, C.POINTER(i32)]
    L.drfe_lsd_extract.argtypes = [vp, vp, i32, i32, sz, i32, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.drfe_lsd_stages.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.drfe_voc_upload.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.drfe_bow_transform_batch.argtypes = [vp, i32, i32, vp]
    L.drfe_bow_download.argtypes = [vp, i32, vp, vp, vp, i32]
    L.drfe_search_by_bow.argtypes = [vp, i32, i32, vp, i32, f32, i32, vp, i32, C.POINTER(i32)]
    L.drfe_planes_ahc.argtypes = [vp, vp, i32, i32, sz, vp, f32, vp, i32, C.POINTER(i32), vp, vp, vp]
    L.drfe_planes_ahc_blocks.argtypes = [vp, vp, i32, i32, sz, vp, f32, vp, vp, i32]
    L.drfe_planes_cape.argtypes = [vp, vp, i32, i32, sz, vp, i32, f32, f32, vp, i32, C.POINTER(i32), vp, vp, vp, vp]
    f64 = C.c_double
    L.drfe_plane_voxel_grid.argtypes = [vp, i32, f32, vp, i32, C.POINTER(i32)]
    L.drfe_plane_refit.argtypes = [vp, vp, i32, f64, C.POINTER(i32)]
    L.drfe_planes_ahc_postprocess.argtypes = [vp, vp, i32, i32, sz, vp, f32, vp, i32, vp, vp, f32, f64, vp, vp, vp, i32,
                                              C.POINTER(i32), C.POINTER(i32)]
    L.drfe_planes_ahc_post_batch.argtypes = [vp, vp, sz, i32, i32, sz, i32, vp, f32, f32, f64, vp, i32, vp, vp, vp, vp, vp, i32]
    L.drfe_debug_ahc_trials.argtypes = [vp, vp, i32, i32, vp]
    L.drfe_debug_order_sort.argtypes = [vp, sz, i32, i32, i32, C.c_uint32]
    L.drfe_debug_order_sort_heap_max.argtypes = [vp, sz, i32, i32, C.POINTER(sz)]
    L.drfe_debug_device_voxel_grid.argtypes = [vp, vp, vp, i32, f32, i32, i32, vp, vp, vp]
    L.drfe_debug_plane_refit.argtypes = [vp, i32, vp, i32, vp, vp, vp, f32, f64, vp, vp]
    L.drfe_planes_ahc_from_blocks.argtypes = [vp, vp, vp, i32, i32, sz, vp, f32, vp, i32, C.POINTER(i32), vp, vp, vp]
    L.drfe_planes_cape_postprocess.argtypes = [vp, vp, i32, i32, sz, vp, vp, vp, i32, f32, f64, vp, vp, vp, i32,
                                               C.POINTER(i32), C.POINTER(i32)]
    L.drfe_surface_normals.argtypes = [vp, vp, i32, i32, sz, vp, f32, vp, i32, C.POINTER(i32), vp, vp, vp]
    L.drfe_surface_normals_batch.argtypes = [vp, vp, sz, sz, i32, i32, vp, f32, f32, i32, vp]
    L.drfe_surface_normals_download.argtypes = [vp, i32, vp, i32, C.POINTER(i32)]
    L.drfe_manhattan_track_host.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]
    L.drfe_manhattan_track_batch.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp]
    L.drfe_manhattan_download.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_debug_manhattan_math.argtypes = [i32, vp, i32, vp]
    L.drfe_plane_match_host.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, i32, vp, vp, vp, C.POINTER(i32)]
    L.drfe_plane_flag_points_host.argtypes = [vp, vp, i32, vp, vp, i32, vp, C.POINTER(i32)]
    L.drfe_plane_match_status_host.argtypes = [vp, vp, vp, i32, vp, vp, i32, vp, C.POINTER(i32)]
    L.drfe_plane_map_upload.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.drfe_plane_match_batch.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.drfe_plane_match_download.argtypes = [vp, i32, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.drfe_plane_flags_download.argtypes = [vp, i32, vp]
    L.drfe_map_plane_update_host.argtypes = [vp, vp, i32, vp, i32, vp, i32, C.POINTER(i32)]
    L.drfe_map_plane_rebuild_host.argtypes = [i32, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.drfe_plane_map_update_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.drfe_plane_map_rebuild_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.drfe_plane_map_edit.argtypes = [vp, i32, i32, vp, vp, vp]
    L.drfe_plane_map_cloud_download.argtypes = [vp, i32, i32, vp, i32, C.POINTER(i32)]
    L.drfe_plane_map_update_stats.argtypes = [vp, vp]
    L.drfe_plane_map_cull_host.argtypes = [C.POINTER(PlaneCullIn), vp, vp, vp, vp, C.POINTER(PlaneCullOut)]
    L.drfe_plane_map_cull_batch.argtypes = [vp, i32, C.POINTER(PlaneCullIn), i32, C.POINTER(PlaneCullOut), vp]
    L.drfe_plane_map_cull_limits.argtypes = [vp]
    L.drfe_plane_map_cull_stats.argtypes = [vp, vp]
    L.drfe_map_point_upkeep_host.argtypes = [i32, vp, vp, vp]
    L.drfe_map_line_upkeep_host.argtypes = [i32, vp, vp, vp]
    L.drfe_map_point_upkeep_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_map_line_upkeep_batch.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_map_upkeep_stats.argtypes = [vp, vp]
    L.drfe_triangulate_points_host.argtypes = [i32, vp, vp, vp, vp]
    L.drfe_triangulate_lines_host.argtypes = [i32, vp, vp, vp, vp]
    L.drfe_triangulate_points_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.drfe_triangulate_lines_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.drfe_triangulate_stats.argtypes = [vp, vp]
    L.drfe_debug_triangulate_math.argtypes = [i32, vp, vp, i32, vp]
    L.drfe_debug_triangulate_math_device.argtypes = [vp, i32, vp, vp, i32, vp]
    L.drfe_sim3_ransac_host.argtypes = [vp, vp]
    L.drfe_sim3_ransac_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_sim3_stats.argtypes = [vp, vp]
    L.drfe_debug_sim3_atan2.argtypes = [vp, vp, i32, vp, vp]
    L.drfe_debug_sim3_rand.argtypes = [C.c_uint32, i32, vp]
    L.drfe_debug_sim3_horn.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.drfe_debug_sim3_hand_back.argtypes = [vp, i32]
    L.drfe_pnp_ransac_host.argtypes = [vp, vp]
    L.drfe_init_ransac_host.argtypes = [vp, vp]
    L.drfe_init_ransac_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_init_stats.argtypes = [vp, vp]
    L.drfe_debug_init_cos_keys.argtypes = [vp, i32, vp, vp]
    L.drfe_debug_init_null_vectors.argtypes = [vp, i32, vp, vp]
    L.drfe_debug_init_check_rt.argtypes = [vp, vp, vp, vp, C.c_float, vp, i32, vp, vp, vp, vp, vp, vp]
    L.drfe_pnp_ransac_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_pose_opt_host.argtypes = [vp, vp]
    L.drfe_pose_opt_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_pose_opt_stats.argtypes = [vp, vp]
    L.drfe_debug_cr_cube.argtypes = [vp, i32, vp, vp]
    L.drfe_debug_pose_opt_ldlt.argtypes = [vp, vp, vp, vp]
    L.drfe_debug_pose_opt_hand_back.argtypes = [vp, i32]
    L.drfe_debug_pose_opt_plane_error.argtypes = [i32, vp, vp, vp, vp]
    L.drfe_trans_opt_host.argtypes = [vp, vp]
    L.drfe_trans_opt_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_trans_opt_stats.argtypes = [vp, vp]
    L.drfe_debug_trans_opt_hand_back.argtypes = [vp, i32]
    L.drfe_debug_trans_opt_plane_error.argtypes = [i32, vp, vp, vp, vp]
    L.drfe_sim3_opt_host.argtypes = [vp, vp]
    L.drfe_sim3_opt_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_sim3_opt_stats.argtypes = [vp, vp]
    L.drfe_debug_sim3_opt_ldlt.argtypes = [vp, vp, vp, vp]
    L.drfe_debug_sim3_opt_step.argtypes = [vp, vp, i32, i32, vp, vp]
    L.drfe_debug_sim3_opt_hand_back.argtypes = [vp, i32]
    L.drfe_kfdb_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.drfe_kfdb_destroy.argtypes = [vp]
    L.drfe_kfdb_destroy.restype = None
    L.drfe_kfdb_last_error.argtypes = [vp]
    L.drfe_kfdb_last_error.restype = C.c_char_p
    L.drfe_kfdb_put.argtypes = [vp, i32, i32, vp, vp]
    for name in ("add", "erase", "remove"):
        getattr(L, "drfe_kfdb_" + name).argtypes = [vp, i32]
    L.drfe_kfdb_clear.argtypes = [vp]
    L.drfe_kfdb_set_neighbours.argtypes = [vp, i32, vp, vp]
    L.drfe_kfdb_size.argtypes = [vp, vp]
    for kind in ("loop", "reloc"):
        getattr(L, f"drfe_kfdb_{kind}_queries_host").argtypes = [vp, vp, vp]
        getattr(L, f"drfe_kfdb_{kind}_queries_device").argtypes = [vp, vp, vp, vp]
        getattr(L, f"drfe_kfdb_{kind}_queries_batch").argtypes = [vp, vp, vp, vp]
    L.drfe_kfdb_score.argtypes = [i32, vp, vp, i32, vp, vp, vp]
    L.drfe_kfdb_stats.argtypes = [vp, vp]
    L.drfe_lmap_create.argtypes = [vp, C.POINTER(vp)]
    L.drfe_lmap_destroy.argtypes = [vp]
    L.drfe_lmap_destroy.restype = None
    L.drfe_lmap_last_error.argtypes = [vp]
    L.drfe_lmap_last_error.restype = C.c_char_p
    L.drfe_lmap_configure.argtypes = [vp, C.c_int64]
    L.drfe_lmap_limits.argtypes = [vp]
    L.drfe_lmap_set_keyframes.argtypes = [vp, vp]
    L.drfe_lmap_set_points.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_lmap_set_lines.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_set_bad.argtypes = [vp, i32, i32, vp, vp]
    L.drfe_lmap_remove.argtypes = [vp, i32, i32]
    L.drfe_lmap_size.argtypes = [vp, vp]
    L.drfe_lmap_update_host.argtypes = [vp, vp, vp]
    L.drfe_lmap_update_device.argtypes = [vp, vp, vp, vp]
    L.drfe_lmap_update_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_lmap_stats.argtypes = [vp, vp]
    L.drfe_lmap_set_connections.argtypes = [vp, vp]
    L.drfe_lmap_get_connections.argtypes = [vp, i32, vp, vp, i32, vp, vp]
    L.drfe_lmap_connect_host.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_connect_device.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_lmap_connect_batch.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_lmap_connect_limits.argtypes = [vp]
    L.drfe_lmap_connect_stats.argtypes = [vp, vp]
    L.drfe_lmap_set_scales.argtypes = [vp, i32, vp]
    L.drfe_lmap_get_scales.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_set_poses.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_get_poses.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_lmap_set_point_geometry.argtypes = [vp, vp]
    L.drfe_lmap_get_point_geometry.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.drfe_lmap_correct_host.argtypes = [vp, i32, vp, i32, vp, vp]
    L.drfe_lmap_correct_device.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.drfe_lmap_correct_batch.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.drfe_lmap_correct_limits.argtypes = [vp]
    L.drfe_lmap_correct_scratch.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_correct_stats.argtypes = [vp, vp]
    L.drfe_lmap_set_cull_attributes.argtypes = [vp, vp]
    L.drfe_lmap_get_cull_attributes.argtypes = [vp, vp]
    L.drfe_lmap_cull_host.argtypes = [vp, i32, vp, i32, vp]
    L.drfe_lmap_cull_device.argtypes = [vp, i32, vp, i32, vp, vp]
    L.drfe_lmap_cull_batch.argtypes = [vp, i32, vp, i32, vp, vp]
    L.drfe_lmap_cull_limits.argtypes = [vp]
    L.drfe_lmap_cull_scratch.argtypes = [vp, i32, vp, vp]
    L.drfe_lmap_cull_stats.argtypes = [vp, vp]
    L.drfe_lmap_upload_bytes.argtypes = [vp, vp]
    L.drfe_lmap_set_gba_keyframes.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_lmap_set_gba_points.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_lmap_get_gba_keyframes.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.drfe_lmap_get_gba_points.argtypes = [vp, i32, vp, vp, vp, vp]
    L.drfe_lmap_gba_host.argtypes = [vp, i32, i32, vp, vp]
    L.drfe_lmap_gba_device.argtypes = [vp, i32, i32, vp, vp, vp]
    L.drfe_lmap_gba_batch.argtypes = [vp, i32, i32, vp, vp, vp]
    L.drfe_lmap_gba_limits.argtypes = [vp]
    L.drfe_lmap_gba_scratch.argtypes = [vp, vp]
    L.drfe_lmap_gba_stats.argtypes = [vp, vp]
    L.drfe_lmap_set_recent_attributes.argtypes = [vp, vp]
    L.drfe_lmap_get_recent_attributes.argtypes = [vp, vp]
    L.drfe_lmap_recent_increase.argtypes = [vp, i32, i32, vp, vp, vp]
    L.drfe_lmap_recent_cull_host.argtypes = [vp, C.c_int64, i32, vp, vp]
    L.drfe_lmap_recent_cull_device.argtypes = [vp, C.c_int64, i32, vp, vp, vp]
    L.drfe_lmap_recent_cull_batch.argtypes = [vp, C.c_int64, i32, vp, vp, vp]
    L.drfe_lmap_recent_cull_limits.argtypes = [vp]
    L.drfe_lmap_recent_cull_scratch.argtypes = [vp, C.c_int64, vp]
    L.drfe_lmap_recent_cull_stats.argtypes = [vp, vp]
    L.drfe_lmap_recent_upload_bytes.argtypes = [vp, vp]
    L.drfe_lmap_fuse_host.argtypes = [vp, vp]
    L.drfe_lmap_fuse_device.argtypes = [vp, vp, vp]
    L.drfe_lmap_fuse_batch.argtypes = [vp, vp, vp]
    L.drfe_lmap_fuse_limits.argtypes = [vp]
    L.drfe_lmap_fuse_scratch.argtypes = [vp, C.c_int64, C.c_int64, vp]
    L.drfe_lmap_fuse_stats.argtypes = [vp, vp]
    L.drfe_lmap_insert_host.argtypes = [vp, vp]
    L.drfe_lmap_insert_device.argtypes = [vp, vp, vp]
    L.drfe_lmap_insert_batch.argtypes = [vp, vp, vp]
    L.drfe_lmap_insert_limits.argtypes = [vp]
    L.drfe_lmap_insert_scratch.argtypes = [vp, i32, vp, i32, vp]
    L.drfe_lmap_insert_stats.argtypes = [vp, vp]
    L.drfe_lmap_create_host.argtypes = [vp, vp]
    L.drfe_lmap_create_device.argtypes = [vp, vp, vp]
    L.drfe_lmap_create_batch.argtypes = [vp, vp, vp]
    L.drfe_lmap_create_limits.argtypes = [vp]
    L.drfe_lmap_create_scratch.argtypes = [vp, i32, i32, vp]
    L.drfe_lmap_create_stats.argtypes = [vp, vp]
    L.drfe_lmap_set_loop_edges.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_lmap_get_loop_edges.argtypes = [vp, i32, vp, i32, vp, vp]
    L.drfe_lmap_essential_upload_bytes.argtypes = [vp, vp]
    L.drfe_lmap_essential_edges_host.argtypes = [vp, vp]
    L.drfe_lmap_essential_edges_device.argtypes = [vp, vp, vp]
    L.drfe_lmap_essential_edges_batch.argtypes = [vp, vp, vp]
    L.drfe_lmap_essential_commit_host.argtypes = [vp, vp]
    L.drfe_lmap_essential_commit_device.argtypes = [vp, vp, vp]
    L.drfe_lmap_essential_commit_batch.argtypes = [vp, vp, vp]
    L.drfe_lmap_essential_limits.argtypes = [vp]
    L.drfe_lmap_essential_scratch.argtypes = [vp, i32, vp]
    L.drfe_lmap_essential_stats.argtypes = [vp, vp]
    L.drfe_lmap_get_replaced.argtypes = [vp, i32, i32, vp, vp]
    L.drfe_lmap_get_match_row.argtypes = [vp, i32, i32, i32, vp, vp]
    L.drfe_lmap_get_observers.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    L.drfe_pnp_stats.argtypes = [vp, vp]
    L.drfe_lines_is_good_batch.argtypes = [vp, vp, vp, vp]
    L.drfe_line3d_chunk_frames.argtypes = [i32]
    L.drfe_line3d_stats.argtypes = [vp, vp]
    L.drfe_debug_pnp_svd.argtypes = [vp, i32, i32, vp, vp, vp]
    L.drfe_debug_pnp_inliers.argtypes = [vp, vp, vp, vp, vp, vp, i32, vp]
    L.drfe_debug_pnp_inliers_device.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    L.drfe_lsd_segments_host.argtypes = [vp, vp, vp, i32, i32, f64, vp, i32, C.POINTER(i32)]
    L.drfe_lsd_configure.argtypes = [vp, i32]
    L.drfe_lsd_configure_rect.argtypes = [vp, i32]
    L.drfe_shard_unique_id.argtypes = [vp]
    L.drfe_shard_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.drfe_shard_destroy.argtypes = [vp]
    L.drfe_shard_destroy.restype = None
    L.drfe_shard_broadcast.argtypes = [vp, vp, sz, i32]
    L.drfe_shard_reduce_report.argtypes = [vp, vp, i32, vp, i32]
    L.drfe_shard_sequences_of_rank.argtypes = [i32, i32, i32, vp, i32]
    L.drfe_shard_last_error.argtypes = [vp]
    L.drfe_shard_last_error.restype = C.c_char_p
    L.drfe_planes_configure_cape.argtypes = [vp, i32]
    L.drfe_planes_cape_stats.argtypes = [vp, vp]
    L.drfe_planes_ahc_stats.argtypes = [vp, vp]
    L.drfe_planes_configure_refit.argtypes = [vp, i32]
    L.drfe_planes_refit_stats.argtypes = [vp, vp]
    L.drfe_frame_load.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, vp]
    L.drfe_bow_transform_slot.argtypes = [vp, i32, i32, vp]
    L.drfe_lsd_configure_nfa.argtypes = [vp, i32]
    L.drfe_lsd_stats.argtypes = [vp, vp]
    L.drfe_long_kernel_clock.argtypes = [vp, i32]
    L.drfe_long_kernel_ms.argtypes = [vp, vp]
    L.drfe_lsd_segments_host_mode.argtypes = [vp, vp, vp, i32, i32, f64, i32, vp, i32, C.POINTER(i32)]
    L.drfe_planes_configure.argtypes = [vp, i32]
    L.drfe_planes_configure_extractor.argtypes = [vp, i32]
    L.drfe_planes_cape_batch.argtypes = [vp, vp, sz, i32, i32, sz, i32, vp, i32, f32, f32, vp, i32, vp, vp, i32]
    L.drfe_batch_status_async.argtypes = [vp, vp, vp]
    L.drfe_batch_check.argtypes = [vp]
    L.drfe_debug_cr_sincos.argtypes = [vp, i32, vp, vp, vp]
    L.drfe_debug_device_order_sort.argtypes = [vp, vp, sz, C.POINTER(i32)]
    L.drfe_debug_device_order_sort_depth.argtypes = [vp, vp, sz, i32, C.POINTER(i32)]
    L.drfe_profile_enable.argtypes = [vp, i32]
    L.drfe_profile_stage_ms.argtypes = [vp, vp]
    L.drfe_stream_sync.argtypes = [vp]
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def quadtree_plan(width, height, nfeatures=1000, scale_factor=1.2, nlevels=8, nframes=512, force=None):
    """How a batch of nframes frames runs k_quadtree (host code, no device): one dict per level with the instantiation's
    threads, kpt (candidate keys a thread keeps in registers) and maxn (node-list capacity), the level's kp_cap and the
    index of its launch.  force: the text of DRFE_QT_FORCE ("<threads>,<kpt>", or one pair per level separated by ';')."""
    L = load()
    # the arguments are set here, not in load(): a variant build from before this entry still loads (tools/bench_variant.py)
    L.drfe_orb_quadtree_plan.argtypes = [C.POINTER(Config), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_void_p]
    cfg = Config(0, int(width), int(height), int(nframes), int(nfeatures), float(scale_factor), int(nlevels), 20, 7)
    out = np.zeros((int(nlevels), 5), np.int32)
    rc = L.drfe_orb_quadtree_plan(C.byref(cfg), int(width), int(height), int(nframes),
                                  None if force is None else str(force).encode(), _p(out))
    if rc < 0:
        raise DrfeError(f"drfe_orb_quadtree_plan failed ({rc})")
    return [dict(level=l, threads=int(r[0]), kpt=int(r[1]), maxn=int(r[2]), kp_cap=int(r[3]), launch=int(r[4]))
            for l, r in enumerate(out)]


def lsd_segments_host(modgrad, angles, cs, max_grad, rect_mode=0):
    """The sequential half of LSD on given level-line fields (host code, no device): [n, 4] float32 segments.
    rect_mode: rect_nfa's reading (0 literal OpenCV 3.4, 1 real-valued)."""
    L = load()
    m = np.ascontiguousarray(modgrad, np.float64)
    a = np.ascontiguousarray(angles, np.float64)
    c = np.ascontiguousarray(cs, np.float32)
    H, W = m.shape
    out = np.zeros((20000, 4), np.float32)
    n = C.c_int()
    rc = L.drfe_lsd_segments_host_mode(_p(m), _p(a), _p(c), W, H, float(max_grad), int(rect_mode), _p(out), len(out), C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_lsd_segments_host failed ({rc})")
    return out[:n.value].copy()


def planes_ahc_from_blocks(blocks17, valid, N, depth16, K4, depth_factor, cap=64):
    """The host half of the AHC extractor on given block fits (no device) -> dict(planes, seg, members)."""
    L = load()
    d = np.ascontiguousarray(depth16, np.uint16)
    h, w = d.shape
    b = np.ascontiguousarray(blocks17, np.float64)
    vn = np.ascontiguousarray(np.stack([valid, N], 1), np.int32)
    planes = np.zeros(cap, PLANE_DTYPE)
    n = C.c_int()
    seg = np.zeros((h, w), np.uint8)
    off = np.zeros(cap + 1, np.int32)
    idx = np.zeros(h * w, np.int32)
    rc = L.drfe_planes_ahc_from_blocks(_p(b), _p(vn), _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)), np.float32(depth_factor),
                                       _p(planes), cap, C.byref(n), _p(seg), _p(off), _p(idx))
    if rc != 0:
        raise DrfeError(f"drfe_planes_ahc_from_blocks failed ({rc})")
    return dict(planes=planes[:n.value].copy(), seg=seg, members=[idx[off[i]:off[i + 1]].copy() for i in range(n.value)])


def plane_voxel_grid(xyz, leaf=0.05):
    """pcl::VoxelGrid(leaf) of an [n, 3] float32 point list (inputCloud order) -> [m, 3] centroids. Host code."""
    L = load()
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    out = np.zeros_like(p)
    n = C.c_int()
    rc = L.drfe_plane_voxel_grid(_p(p), len(p), np.float32(leaf), _p(out), len(p), C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_plane_voxel_grid failed ({rc})")
    return out[:n.value].copy()


def plane_refit(coef4, xyz, dist_threshold):
    """Frame::MaxPointDistanceFromPlane(coef, cloud) -> (valid, coef after the refit). Host code."""
    L = load()
    c = np.ascontiguousarray(coef4, np.float32).copy()
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    v = C.c_int()
    rc = L.drfe_plane_refit(_p(c), _p(p), len(p), float(dist_threshold), C.byref(v))
    if rc != 0:
        raise DrfeError(f"drfe_plane_refit failed ({rc})")
    return bool(v.value), c


def debug_order_sort_heap_max(recs, kind, depth_limit=-1):
    """Test hook: uint32 keys (kind 0) / uint64 records (kind 1) through the plain transcription of libstdc++'s introsort
    (drfe_debug_order_sort mode 3) -> (sorted copy, longest range that reached std::__partial_sort or 0).  Host code."""
    L = load()
    r = np.ascontiguousarray(recs, np.uint32 if kind == 0 else np.uint64).copy()
    longest = C.c_size_t(0)
    rc = L.drfe_debug_order_sort_heap_max(_p(r), len(r), kind, depth_limit, C.byref(longest))
    if rc != 0:
        raise DrfeError(f"drfe_debug_order_sort_heap_max failed ({rc})")
    return r, int(longest.value)


def _csr(clouds):
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds])
    xyz = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if len(clouds) else np.zeros((0, 3)), np.float32)
    return xyz, off


def debug_plane_refit(ctx, on_device, planes, clouds, max_point_dist, dist_threshold, vcounts_override=None):
    """Test hook: gates + refit of hand-built PLANE_DTYPE records, one [n, 3] voxel cloud each, through k_plane_refit (on_device,
    ctx a Context) or the host loop (ctx may be None) -> (post [n_planes] PLANE_POST_DTYPE, status [n_planes + 1]: 0 final,
    1 not certified, 2 grid came back, -1 no such plane - the job past the last plane)."""
    L = load()
    pl = np.ascontiguousarray(planes, PLANE_DTYPE)
    xyz, off = _csr(clouds)
    assert len(clouds) == len(pl) >= 1
    ov = None if vcounts_override is None else np.ascontiguousarray(vcounts_override, np.int32)
    post = np.zeros(len(pl), PLANE_POST_DTYPE)
    status = np.full(len(pl) + 1, 99, np.int32)
    rc = L.drfe_debug_plane_refit(ctx.h if ctx is not None else None, 1 if on_device else 0, _p(pl), len(pl), _p(xyz), _p(off), _p(ov) if ov is not None else None,
                                  np.float32(max_point_dist), float(dist_threshold), _p(post), _p(status))
    if rc != 0:
        raise DrfeError(f"drfe_debug_plane_refit failed ({rc}): {ctx.last_error() if ctx is not None else ''}")
    return post, status


def manhattan_track_host(R, recs, line_dirs=None, n_calls=3):
    """Tracking::TrackManhattanFrame chained n_calls times on one frame's SurfaceNormal records (SURFACE_NORMAL_DTYPE) and
    optional line directions (n x 3 float64).  Returns (R_out 3x3 float32, info (MANHATTAN_INFO_DTYPE), rec_bits uint16,
    line_bits uint16)."""
    L = load()
    R = np.ascontiguousarray(R, np.float32).reshape(3, 3)
    recs = np.ascontiguousarray(recs, SURFACE_NORMAL_DTYPE)
    dirs = np.ascontiguousarray(np.zeros((0, 3)) if line_dirs is None else line_dirs, np.float64).reshape(-1, 3)
    out = np.zeros((3, 3), np.float32)
    info = np.zeros((), MANHATTAN_INFO_DTYPE)
    rb = np.zeros(len(recs), np.uint16)
    lb = np.zeros(len(dirs), np.uint16)
    rc = L.drfe_manhattan_track_host(_p(R), _p(recs), len(recs), _p(dirs), len(dirs), n_calls, _p(out), _p(info), _p(rb), _p(lb))
    if rc != 0:
        raise DrfeError(f"drfe_manhattan_track_host failed ({rc})")
    return out, info, rb, lb


def _plane_params(params):
    return np.ascontiguousarray(PLANE_MATCH_DEFAULTS if params is None else params, np.float32).reshape(4)


def _clouds_csr(clouds):
    """list of [n, 3] clouds -> (offsets int32[len + 1], xyz float32[total, 3])"""
    off = np.zeros(len(clouds) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in clouds]) if len(clouds) else []
    xyz = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]) if len(clouds) else np.zeros((0, 3), np.float32)
    return off, np.ascontiguousarray(xyz, np.float32)


def _priors(p, n):
    return np.full(n, -1, np.int32) if p is None else np.array(p, np.int32).reshape(n)


def plane_match_host(Tcw, coefs, map_coefs, map_bad, clouds, map_idx=None, par_idx=None, ver_idx=None, params=None):
    """PlaneMatcher::SearchMapByCoefficients on one frame (host entry): Tcw 4x4, coefs [P, 4] camera-frame planes, map planes
    map_coefs [M, 4] (world), map_bad [M], clouds (list of M [n, 3] arrays); the three prior index arrays (None = all -1).
    Returns (map_idx, par_idx, ver_idx, nmatches)."""
    L = load()
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    cf = np.ascontiguousarray(coefs, np.float32).reshape(-1, 4)
    mc = np.ascontiguousarray(map_coefs, np.float32).reshape(-1, 4)
    bad = np.ascontiguousarray(map_bad, np.uint8).reshape(len(mc))
    off, xyz = _clouds_csr(clouds)
    assert len(off) == len(mc) + 1
    P = len(cf)
    mi, pi, vi = _priors(map_idx, P), _priors(par_idx, P), _priors(ver_idx, P)
    n = C.c_int()
    prm = _plane_params(params)
    rc = L.drfe_plane_match_host(_p(prm), _p(T), _p(cf), P, _p(mc), _p(bad), _p(off), _p(xyz), len(mc), _p(mi), _p(pi), _p(vi),
                                 C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_plane_match_host failed ({rc})")
    return mi, pi, vi, n.value


def plane_flag_points_host(Tcw, coefs, map_idx, points, flags=None):
    """Map::FlagMatchedPlanePoints on one frame (host entry): flags (uint8 per map point, OR-ed into `flags` when given) and
    the (plane, point) pair count."""
    L = load()
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    cf = np.ascontiguousarray(coefs, np.float32).reshape(-1, 4)
    mi = np.ascontiguousarray(map_idx, np.int32).reshape(len(cf))
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    fl = np.zeros(len(pts), np.uint8) if flags is None else np.array(flags, np.uint8).reshape(len(pts))
    n = C.c_int()
    rc = L.drfe_plane_flag_points_host(_p(T), _p(cf), len(cf), _p(mi), _p(pts), len(pts), _p(fl), C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_plane_flag_points_host failed ({rc})")
    return fl, n.value


def plane_match_status_host(Tcw, coefs, matched_coefs, matched, mf_contrast, Rwc_MF=None, params=None):
    """PlaneMatcher::bMatchStatus on one frame (host entry): matched_coefs [P, 4] world coefficients of mvpMapPlanes[i],
    matched [P] (0 = null or bad).  Returns the bool result."""
    L = load()
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    cf = np.ascontiguousarray(coefs, np.float32).reshape(-1, 4)
    mc = np.ascontiguousarray(matched_coefs, np.float32).reshape(len(cf), 4)
    m = np.ascontiguousarray(matched, np.uint8).reshape(len(cf))
    R = None if Rwc_MF is None else np.ascontiguousarray(Rwc_MF, np.float32).reshape(9)
    st = C.c_int()
    prm = _plane_params(params)
    rc = L.drfe_plane_match_status_host(_p(prm), _p(T), _p(cf), len(cf), _p(mc), _p(m), int(bool(mf_contrast)), _p(R), C.byref(st))
    if rc != 0:
        raise DrfeError(f"drfe_plane_match_status_host failed ({rc})")
    return bool(st.value)


def map_plane_update_host(Tcw, frame_xyz, map_xyz):
    """MapPlane::UpdateCoefficientsAndPoints(F, i) (host entry): VoxelGrid(0.05) of frame_xyz [n, 3] moved into world by
    Isometry3d(toSE3Quat(Tcw)).inverse(), followed by the plane's cloud map_xyz [m, 3].  Returns the new cloud [k, 3]."""
    L = load()
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    fx = np.ascontiguousarray(frame_xyz, np.float32).reshape(-1, 3)
    mx = np.ascontiguousarray(map_xyz, np.float32).reshape(-1, 3)
    out = np.zeros((len(fx) + len(mx), 3), np.float32)
    n = C.c_int()
    rc = L.drfe_map_plane_update_host(_p(T), _p(fx), len(fx), _p(mx), len(mx), _p(out), len(out), C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_map_plane_update_host failed ({rc})")
    return out[:n.value].copy()


def map_plane_rebuild_host(Twc, clouds):
    """MapPlane::UpdateCoefficientsAndPoints() (host entry): VoxelGrid(0.05) of the observations' clouds (list of [n, 3]) moved
    by their Twc (list of 4x4, widened element by element), concatenated in the order given.  Returns the new cloud [k, 3]."""
    L = load()
    T = np.ascontiguousarray(np.asarray(Twc, np.float32).reshape(-1, 16), np.float32)
    off, xyz = _clouds_csr(clouds)
    assert len(T) == len(clouds)
    out = np.zeros((max(len(xyz), 1), 3), np.float32)
    n = C.c_int()
    rc = L.drfe_map_plane_rebuild_host(len(clouds), _p(T), _p(off), _p(xyz), _p(out), len(xyz), C.byref(n))
    if rc != 0:
        raise DrfeError(f"drfe_map_plane_rebuild_host failed ({rc})")
    return out[:n.value].copy()


class PlaneCullIn(C.Structure):
    _fields_ = [("n_planes", C.c_int32), ("n_kfs", C.c_int32), ("n_recent", C.c_int32), ("current_kf_id", C.c_int32),
                ("dTh", C.c_double), ("aTh", C.c_double)] + [(k, C.c_void_p) for k in (
        "found", "visible", "n_obs", "first_kf_id", "obs_offsets", "obs_kf", "obs_idx", "obs_cloud", "obs_cloud_n")] + [
        ("obs_cloud_stride", C.c_int32), ("Twc", C.c_void_p), ("recent", C.c_void_p)]      # drfe_plane_cull_in


class PlaneCullOut(C.Structure):
    _fields_ = [("n_events", C.c_int32), ("n_rebuilt", C.c_int32)] + [(k, C.c_void_p) for k in (
        "events", "bad", "n_obs", "found", "visible", "rebuilt", "rebuilt_offsets", "rebuilt_xyz")] + [
        ("rebuilt_capacity", C.c_int32), ("verdicts", C.c_void_p), ("counters", C.c_int64 * 4)]   # drfe_plane_cull_out


# DRFE_PLANE_CULL_*: the verdict of one entry of mlpRecentAddedMapPlanes
PLANE_CULL_KEPT, PLANE_CULL_ERASED_BAD, PLANE_CULL_BAD_BY_RATIO, PLANE_CULL_BAD_BY_OBSERVATIONS, PLANE_CULL_ERASED_BY_AGE = range(5)
PLANE_CULL_COUNTERS = ("gated_pairs", "pair_points", "rebuilds", "stale_columns")
PLANE_CULL_STATS = ("calls", "device_calls", "dist_launches", "rebuild_calls")
PLANE_CULL_DISPATCH, PLANE_CULL_DEVICE, PLANE_CULL_HOST_WALK, PLANE_CULL_DEVICE_PER_PAIR = range(4)   # drfe_plane_map_cull_batch's mode
PLANE_CULL_DEVICE_FROM = 16385                                                       # DRFE_PLANE_CULL_DEVICE_FROM
PLANE_CULL_CLOUD_STRIDE = 16         # the bytes between the points of an observation cloud as the wrappers pack them (PointXYZ)


def _plane_cull_pack(scene, rebuilt_capacity=None):
    """A culling scene (dict: found / visible / n_obs / first_kf_id [P], obs = per plane a list of (key frame, plane in it) in
    key-frame order, kf_clouds = per key frame a list of [n, 3] clouds, Twc [K, 4, 4], dTh, aTh, current_kf_id, recent) ->
    (drfe_plane_cull_in, drfe_plane_cull_out, the arrays they point to, the output arrays)"""
    P = len(scene["found"])
    K = len(scene["kf_clouds"])
    keep = {}
    for k in ("found", "visible", "n_obs", "first_kf_id"):
        keep[k] = np.ascontiguousarray(scene[k], np.int32).reshape(P)
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum([len(o) for o in scene["obs"]]) if P else []
    flat = [o for obs in scene["obs"] for o in obs]
    keep["obs_offsets"] = off
    keep["obs_kf"] = np.ascontiguousarray([o[0] for o in flat], np.int32)
    keep["obs_idx"] = np.ascontiguousarray([o[1] for o in flat], np.int32)
    # every key-frame cloud padded to PointXYZ's 16 bytes, the pad poisoned: only x y z may be read
    padded = {}
    for kf, idx in flat:
        if (kf, idx) not in padded:
            c = np.asarray(scene["kf_clouds"][kf][idx], np.float32).reshape(-1, 3)
            q = np.full((max(len(c), 1), 4), np.nan, np.float32)
            q[:len(c), :3] = c
            padded[(kf, idx)] = (q, len(c))
    keep["padded"] = padded
    keep["obs_cloud"] = np.ascontiguousarray([padded[o][0].ctypes.data for o in flat], np.uint64)
    keep["obs_cloud_n"] = np.ascontiguousarray([padded[o][1] for o in flat], np.int32)
    keep["Twc"] = np.ascontiguousarray(np.asarray(scene["Twc"], np.float32).reshape(-1, 16), np.float32)
    assert len(keep["Twc"]) == K
    keep["recent"] = np.ascontiguousarray(scene["recent"], np.int32).reshape(-1)
    cin = PlaneCullIn(P, K, len(keep["recent"]), int(scene["current_kf_id"]), float(scene["dTh"]), float(scene["aTh"]))
    for k in ("found", "visible", "n_obs", "first_kf_id", "obs_offsets", "obs_kf", "obs_idx", "obs_cloud", "obs_cloud_n", "Twc", "recent"):
        setattr(cin, k, _p(keep[k]) if keep[k].size else None)
    cin.obs_offsets = _p(off)
    cin.obs_cloud_stride = PLANE_CULL_CLOUD_STRIDE
    cap = int(keep["obs_cloud_n"].sum()) if rebuilt_capacity is None else int(rebuilt_capacity)
    o = dict(events=np.zeros((max(P, 1), 2), np.int32), bad=np.zeros(max(P, 1), np.uint8), n_obs=np.zeros(max(P, 1), np.int32),
             found=np.zeros(max(P, 1), np.int32), visible=np.zeros(max(P, 1), np.int32), rebuilt=np.zeros(max(P, 1), np.int32),
             rebuilt_offsets=np.zeros(P + 1, np.int32), rebuilt_xyz=np.zeros((max(cap, 1), 3), np.float32),
             verdicts=np.zeros(max(len(keep["recent"]), 1), np.uint8))
    cout = PlaneCullOut()
    for k, a in o.items():
        setattr(cout, k, _p(a))
    cout.rebuilt_capacity = cap
    return cin, cout, keep, o


def _plane_cull_result(cin, cout, o):
    P, E, R = cin.n_planes, cout.n_events, cout.n_rebuilt
    off = o["rebuilt_offsets"]
    return dict(events=o["events"][:E].copy(), bad=o["bad"][:P].copy(), n_obs=o["n_obs"][:P].copy(), found=o["found"][:P].copy(),
                visible=o["visible"][:P].copy(), rebuilt=o["rebuilt"][:R].tolist(),
                clouds={int(o["rebuilt"][k]): o["rebuilt_xyz"][off[k]:off[k + 1]].copy() for k in range(R)},
                verdicts=o["verdicts"][:cin.n_recent].copy(), counters=dict(zip(PLANE_CULL_COUNTERS, list(cout.counters))))


def plane_map_cull_host(scene, rebuilt_capacity=None):
    """LocalMapping::MapPlaneCulling on the host (drfe_plane_map_cull_host): scene as _plane_cull_pack takes it plus coefs [P, 4],
    bad [P] and clouds (list of P [n, 3]).  Returns dict(events [E, 2] (replaced, survivor), bad, n_obs, found, visible, rebuilt,
    clouds {plane: [n, 3]}, verdicts, counters)."""
    L = load()
    cin, cout, keep, o = _plane_cull_pack(scene, rebuilt_capacity)
    coefs = np.ascontiguousarray(scene["coefs"], np.float32).reshape(-1, 4)
    bad = np.ascontiguousarray(scene["bad"], np.uint8).reshape(-1)
    coff, xyz = _clouds_csr(list(scene["clouds"]))
    assert len(coefs) == len(bad) == len(scene["clouds"]) == cin.n_planes
    rc = L.drfe_plane_map_cull_host(C.byref(cin), _p(coefs), _p(bad), _p(coff), _p(xyz), C.byref(cout))
    if rc != 0:
        raise DrfeError(f"drfe_plane_map_cull_host failed ({rc})")
    return _plane_cull_result(cin, cout, o)


def plane_map_cull_limits():
    """dict(chunk, row_tile, device_from, max_planes) of the device culling pass"""
    out = np.zeros(4, np.int32)
    rc = load().drfe_plane_map_cull_limits(_p(out))
    if rc != 0:
        raise DrfeError(f"drfe_plane_map_cull_limits failed ({rc})")
    return dict(zip(("chunk", "row_tile", "device_from", "max_planes"), out.tolist()))


def _upkeep_call(fn, head, line, scene, what, frustum):
    """Packs a scene (dict: kf_center [K, 3], kf_bad [K] or None, scale_factors [L], bad [n] or None, obs_offsets [n + 1],
    obs_kf [T], obs_desc [T, 32], world [n, 3] float32 (points) / [n, 6] float64 (lines), ref_kf [n], ref_level [n]) into the
    drfe_upkeep_* records, calls fn(*head, what, kfs, items, out) and returns the outputs as a dict."""
    a = {}

    def arr(key, dt, shape=None):
        v = scene.get(key)
        if v is None:
            return None
        v = np.ascontiguousarray(v, dt)
        a[key] = v if shape is None else v.reshape(shape)
        return a[key]
    off = arr("obs_offsets", np.int32, -1)
    n = len(off) - 1 if off is not None else 0
    cen = arr("kf_center", np.float32, (-1, 3))
    sc = arr("scale_factors", np.float32, -1)
    kfb = arr("kf_bad", np.uint8, -1)
    kfs = UpkeepKeyframes(len(cen), len(sc), _p(cen), _p(kfb), _p(sc))
    items = UpkeepItems(n, 0, _p(arr("bad", np.uint8, -1)), _p(off), _p(arr("obs_kf", np.int32, -1)),
                        _p(arr("obs_desc", np.uint8, (-1, 32))),
                        _p(arr("world", np.float64 if line else np.float32, (-1, 6 if line else 3))),
                        _p(arr("ref_kf", np.int32, -1)), _p(arr("ref_level", np.int32, -1)))
    r = dict(best_obs=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8),
             normal=np.zeros((n, 3), np.float64 if line else np.float32), max_distance=np.zeros(n, np.float32),
             min_distance=np.zeros(n, np.float32), status=np.zeros(n, np.uint8))
    if frustum:
        r["frustum"] = np.zeros(n, FRUSTUM_LINE_DTYPE if line else FRUSTUM_POINT_DTYPE)
    out = UpkeepOut(_p(r["best_obs"]), _p(r["desc"]), _p(r["normal"]), _p(r["max_distance"]), _p(r["min_distance"]),
                    _p(r["status"]), _p(r.get("frustum")))
    rc = fn(*head, int(what), C.byref(kfs), C.byref(items), C.byref(out), *([None] if head else []))
    return rc, r


def map_point_upkeep_host(scene, what=3, frustum=True):
    """MapPoint::ComputeDistinctiveDescriptors (what & 1) + UpdateNormalAndDepth (what & 2) of n map points on the host
    (DESIGN.md section 14); scene as _upkeep_call.  Returns dict(best_obs, desc, normal, max_distance, min_distance, status,
    frustum)."""
    L = load()
    rc, r = _upkeep_call(L.drfe_map_point_upkeep_host, (), False, scene, what, frustum)
    if rc != 0:
        raise DrfeError(f"drfe_map_point_upkeep_host failed ({rc})")
    return r


def map_line_upkeep_host(scene, what=3, frustum=True):
    """MapLine::ComputeDistinctiveDescriptors (what & 1) + UpdateAverageDir (what & 2) of n map lines on the host; as
    map_point_upkeep_host with world [n, 6] float64 and a float64 normal."""
    L = load()
    rc, r = _upkeep_call(L.drfe_map_line_upkeep_host, (), True, scene, what, frustum)
    if rc != 0:
        raise DrfeError(f"drfe_map_line_upkeep_host failed ({rc})")
    return r


def _tri_call(fn, head, line, scene, monocular=0):
    """Packs a scene (dict: kf [K] TRI_KF_DTYPE, scale_factors [K, L], level_sigma2 [K, L], offsets [K + 1]; points: un [F, 2],
    raw [F, 2], octave [F], u_right [F], depth [F]; lines: ends [F, 4], octave [F], depth [F], lines3d [F, 6] float64; pairs:
    kf1 [P], kf2 [P], match_offsets [P + 1], matches [M, 2]) into the drfe_tri_* records, calls
    fn(*head, monocular, kfs, features, pairs, out) and returns the outputs as a dict (status, branch, x3d [M, 3 | 6],
    pair_skipped, accepted)."""
    keep = []

    def arr(key, dt, shape=-1):
        v = scene.get(key)
        if v is None:
            return None
        v = np.ascontiguousarray(np.asarray(v, dt).reshape(shape))
        keep.append(v)
        return v
    kf = np.ascontiguousarray(scene["kf"], TRI_KF_DTYPE)
    keep.append(kf)
    sc = arr("scale_factors", np.float32, (len(kf), -1))
    sg = arr("level_sigma2", np.float32, (len(kf), -1))
    kfs = TriKeyframes(len(kf), sc.shape[1] if sc is not None and len(kf) else 1, _p(kf), _p(sc), _p(sg))
    off = arr("offsets", np.int32)
    if line:
        feats = TriKeylines(_p(off), _p(arr("ends", np.float32, (-1, 4))), _p(arr("octave", np.int32)), _p(arr("depth", np.float32)),
                            _p(arr("lines3d", np.float64, (-1, 6))))
    else:
        feats = TriKeypoints(_p(off), _p(arr("un", np.float32, (-1, 2))), _p(arr("raw", np.float32, (-1, 2))),
                             _p(arr("octave", np.int32)), _p(arr("u_right", np.float32)), _p(arr("depth", np.float32)))
    mo = arr("match_offsets", np.int32)
    P = len(mo) - 1
    M = int(mo[-1])
    pairs = TriPairs(P, 0, _p(arr("kf1", np.int32)), _p(arr("kf2", np.int32)), _p(mo), _p(arr("matches", np.int32, (-1, 2))))
    r = dict(status=np.zeros(M, np.uint8), branch=np.zeros(M, np.uint8), x3d=np.zeros((M, 6 if line else 3), np.float32),
             pair_skipped=np.zeros(P, np.uint8), accepted=np.zeros(P, np.int32))
    out = TriOut(_p(r["status"]), _p(r["branch"]), _p(r["x3d"]), _p(r["pair_skipped"]), _p(r["accepted"]))
    rc = fn(*head, int(monocular), C.byref(kfs), C.byref(feats), C.byref(pairs), C.byref(out), *([None] if head else []))
    return rc, r


def triangulate_points_host(scene, monocular=0):
    """LocalMapping::CreateNewMapPoints' per-match body on the host (drfe_triangulate_points_host);
    scene as _tri_call"""
    rc, r = _tri_call(load().drfe_triangulate_points_host, (), False, scene, monocular)
    if rc != 0:
        raise DrfeError(f"drfe_triangulate_points_host failed ({rc})")
    return r


def triangulate_lines_host(scene, monocular=0):
    """LocalMapping::CreateNewMapLines2's per-match body on the host (drfe_triangulate_lines_host)"""
    rc, r = _tri_call(load().drfe_triangulate_lines_host, (), True, scene, monocular)
    if rc != 0:
        raise DrfeError(f"drfe_triangulate_lines_host failed ({rc})")
    return r


def triangulate_math(which, y, x=None):
    """drfe_atan2f(y, x) (0), drfe_cosf(y) (1), drfe_cosf(2 * drfe_atan2f(y / 2, x)) (2) of include/drfe_math.h, float32"""
    L = load()
    y = np.ascontiguousarray(y, np.float32)
    x = np.ascontiguousarray(np.zeros_like(y) if x is None else x, np.float32)
    out = np.zeros_like(y)
    if L.drfe_debug_triangulate_math(which, _p(y), _p(x), len(y), _p(out)) != 0:
        raise DrfeError("drfe_debug_triangulate_math failed")
    return out


def _sim3_pack(problems):
    """Packs a problem set (dict: Tcw1 [n, 12], Tcw2 [n, 12], K1 [n, 4], K2 [n, 4] (fx, fy, cx, cy), fix_scale [n], probability [n],
    min_inliers [n], max_iterations [n], seed [n], offsets [n + 1], Xw1 [M, 3], Xw2 [M, 3], sigma2_1 [M], sigma2_2 [M]) into
    drfe_sim3_problems and allocates the table: (problems record, out record, the table as a dict, the arrays to keep alive).  The
    table: per solver iterations, hypotheses, row0, words, mask0; per row sample [3], R12 [9], t12 [3], s12, T12 [12], inliers,
    returns, best; mask (uint64 words).  Solver s's rows are row0[s] + h, its mask words mask0[s] + h * words[s] + (i // 64)
    (sim3_table slices them)."""
    keep = []

    def arr(key, dt, shape=-1):
        v = np.ascontiguousarray(np.asarray(problems[key], dt).reshape(shape))
        keep.append(v)
        return v
    off = arr("offsets", np.int32)
    n = len(off) - 1
    maxit = arr("max_iterations", np.int32)
    P = Sim3Problems(n, 0, _p(arr("Tcw1", np.float32, (-1, 12))), _p(arr("Tcw2", np.float32, (-1, 12))),
                     _p(arr("K1", np.float32, (-1, 4))), _p(arr("K2", np.float32, (-1, 4))), _p(arr("fix_scale", np.uint8)),
                     _p(arr("probability", np.float64)), _p(arr("min_inliers", np.int32)), _p(maxit), _p(arr("seed", np.uint32)),
                     _p(off), _p(arr("Xw1", np.float32, (-1, 3))), _p(arr("Xw2", np.float32, (-1, 3))),
                     _p(arr("sigma2_1", np.float32)), _p(arr("sigma2_2", np.float32)))
    cap = np.maximum(maxit.astype(np.int64), 1)
    words = (np.diff(off.astype(np.int64)) + 63) // 64
    row0 = np.concatenate([[0], np.cumsum(cap)])
    mask0 = np.concatenate([[0], np.cumsum(cap * words)])
    rows, W = int(row0[-1]), int(mask0[-1])
    r = dict(iterations=np.zeros(n, np.int32), hypotheses=np.zeros(n, np.int32), row0=row0[:-1], words=words, mask0=mask0[:-1],
             sample=np.zeros((rows, 3), np.int32), R12=np.zeros((rows, 9), np.float32), t12=np.zeros((rows, 3), np.float32),
             s12=np.zeros(rows, np.float32), T12=np.zeros((rows, 12), np.float32), inliers=np.zeros(rows, np.int32),
             returns=np.zeros(rows, np.uint8), best=np.zeros(rows, np.int32), mask=np.zeros(W, np.uint64))
    out = Sim3Out(*[_p(r[k]) for k in ("iterations", "hypotheses", "sample", "R12", "t12", "s12", "T12", "inliers", "returns",
                                       "best", "mask")])
    return P, out, r, keep


def _sim3_call(fn, head, problems):
    """fn(*head, problems, out) over _sim3_pack's records: (return code, table)"""
    P, out, r, _keep = _sim3_pack(problems)
    rc = fn(*head, C.byref(P), C.byref(out), *([None] if head else []))
    return rc, r


def sim3_ransac_host(problems):
    """Sim3Solver's whole hypothesis table of every solver on the host (drfe_sim3_ransac_host);
    problems and result as _sim3_call"""
    rc, r = _sim3_call(load().drfe_sim3_ransac_host, (), problems)
    if rc != 0:
        raise DrfeError(f"drfe_sim3_ransac_host failed ({rc})")
    return r


def sim3_table(result, s):
    """Solver s's filled rows of a sim3_ransac_* result: dict(iterations, sample, R12, t12, s12, T12, inliers, returns, best,
    mask [hypotheses, words])"""
    a, n, w = int(result["row0"][s]), int(result["hypotheses"][s]), int(result["words"][s])
    t = {k: result[k][a:a + n] for k in ("sample", "R12", "t12", "s12", "T12", "inliers", "returns", "best")}
    m0 = int(result["mask0"][s])
    t["mask"] = result["mask"][m0:m0 + n * w].reshape(n, w)
    t["iterations"] = int(result["iterations"][s])
    return t


def _pnp_pack(problems):
    """Packs a problem set (dict: K [n, 4] (fx, fy, cx, cy), probability [n], min_inliers [n], max_iterations [n], epsilon [n],
    th2 [n], tail [n], seed [n], offsets [n + 1], p2d [M, 2], Xw [M, 3], sigma2 [M]) into drfe_pnp_problems and allocates the
    table: (problems record, out record, the table as a dict, the arrays to keep alive).  The table: per solver iterations,
    min_inliers, hypotheses, refines, row0, words, mask0; per row sample [4], R [9], t [3], inliers, best, returns, refined_R,
    refined_t, refined_inliers; mask and refined_mask (uint64 words).  Solver s's rows are row0[s] + h, its mask words
    mask0[s] + h * words[s] + (i // 64) (pnp_table slices them)."""
    keep = []

    def arr(key, dt, shape=-1):
        v = np.ascontiguousarray(np.asarray(problems[key], dt).reshape(shape))
        keep.append(v)
        return v
    off = arr("offsets", np.int32)
    n = len(off) - 1
    maxit, tail = arr("max_iterations", np.int32), arr("tail", np.int32)
    P = PnpProblems(n, 0, _p(arr("K", np.float32, (-1, 4))), _p(arr("probability", np.float64)), _p(arr("min_inliers", np.int32)),
                    _p(maxit), _p(arr("epsilon", np.float32)), _p(arr("th2", np.float32)), _p(tail), _p(arr("seed", np.uint32)),
                    _p(off), _p(arr("p2d", np.float32, (-1, 2))), _p(arr("Xw", np.float32, (-1, 3))), _p(arr("sigma2", np.float32)))
    cap = np.maximum(maxit.astype(np.int64), 1) + np.clip(tail.astype(np.int64), 0, None)
    words = (np.clip(np.diff(off.astype(np.int64)), 0, None) + 63) // 64
    row0 = np.concatenate([[0], np.cumsum(cap)])
    mask0 = np.concatenate([[0], np.cumsum(cap * words)])
    rows, W = int(row0[-1]), int(mask0[-1])
    r = dict(iterations=np.zeros(n, np.int32), min_inliers=np.zeros(n, np.int32), hypotheses=np.zeros(n, np.int32),
             refines=np.zeros(n, np.int32), row0=row0[:-1], words=words, mask0=mask0[:-1],
             sample=np.zeros((rows, 4), np.int32), R=np.zeros((rows, 9), np.float64), t=np.zeros((rows, 3), np.float64),
             inliers=np.zeros(rows, np.int32), mask=np.zeros(W, np.uint64), best=np.zeros(rows, np.int32),
             returns=np.zeros(rows, np.uint8), refined_R=np.zeros((rows, 9), np.float64), refined_t=np.zeros((rows, 3), np.float64),
             refined_inliers=np.zeros(rows, np.int32), refined_mask=np.zeros(W, np.uint64))
    out = PnpOut(*[_p(r[k]) for k in PNP_OUT_FIELDS])
    return P, out, r, keep


def _pnp_call(fn, head, problems):
    """fn(*head, problems, out) over _pnp_pack's records: (return code, table)"""
    P, out, r, _keep = _pnp_pack(problems)
    rc = fn(*head, C.byref(P), C.byref(out), *([None] if head else []))
    return rc, r


def pnp_ransac_host(problems):
    """PnPsolver's whole table of every solver on the host (drfe_pnp_ransac_host); problems and result as
    _pnp_pack"""
    rc, r = _pnp_call(load().drfe_pnp_ransac_host, (), problems)
    if rc != 0:
        raise DrfeError(f"drfe_pnp_ransac_host failed ({rc})")
    return r


def pnp_table(result, s):
    """Solver s's filled rows of a pnp_ransac_* result: dict(iterations, min_inliers, refines, sample, R, t, inliers, best,
    returns, refined_R, refined_t, refined_inliers, mask [rows, words], refined_mask [rows, words])"""
    a, n, w = int(result["row0"][s]), int(result["hypotheses"][s]), int(result["words"][s])
    t = {k: result[k][a:a + n] for k in ("sample", "R", "t", "inliers", "best", "returns", "refined_R", "refined_t",
                                         "refined_inliers")}
    m0 = int(result["mask0"][s])
    for k in ("mask", "refined_mask"):
        t[k] = result[k][m0:m0 + n * w].reshape(n, w)
    for k in ("iterations", "min_inliers", "refines"):
        t[k] = int(result[k][s])
    return t


def _pose_opt_pack(problems):
    """Packs a set of frames (dict: Tcw [n, 16], K [n, 4] (fx, fy, cx, cy), bf [n], b_struct [n], point_offsets [n + 1], obs [P, 2],
    u_right [P], inv_sigma2 [P], Xw [P, 3], line_offsets [n + 1], line_fn [L, 3], line_ends [L, 6]; optional plane_offsets [n + 1],
    plane_meas [S, 4], plane_world [S, 12], plane_mask [S], plane_settings [7]) into drfe_pose_opt_problems and allocates the
    outputs: (problems record, out record, the outputs as a dict, the arrays to keep alive).  The outputs: per frame Tcw [16],
    returns, rounds, iterations, trials, diag [8] (POSE_OPT_DIAG names the first six); per point, line and plane slot the outlier
    flags."""
    keep = []

    def arr(key, dt, shape=-1, default=None):
        v = np.asarray(problems.get(key, default), dt)
        v = np.ascontiguousarray(v.reshape(shape) if v.size else np.zeros((0,) + (shape[1:] if isinstance(shape, tuple) else ()), dt))
        keep.append(v)
        return v
    poff = arr("point_offsets", np.int32)
    n = len(poff) - 1
    loff = arr("line_offsets", np.int32, default=np.zeros(n + 1, np.int32))
    soff = arr("plane_offsets", np.int32, default=np.zeros(n + 1, np.int32))
    nP, nL, nS = (max(int(o[-1]), 0) if len(o) else 0 for o in (poff, loff, soff))
    z = np.zeros(0)
    P = PoseOptProblems(n, 0, _p(arr("Tcw", np.float32, (-1, 16))), _p(arr("K", np.float32, (-1, 4))), _p(arr("bf", np.float32)),
                        _p(arr("b_struct", np.uint8, default=np.zeros(n, np.uint8))), _p(poff),
                        _p(arr("obs", np.float32, (-1, 2), z)), _p(arr("u_right", np.float32, -1, z)),
                        _p(arr("inv_sigma2", np.float32, -1, z)), _p(arr("Xw", np.float32, (-1, 3), z)), _p(loff),
                        _p(arr("line_fn", np.float64, (-1, 3), z)), _p(arr("line_ends", np.float64, (-1, 6), z)), _p(soff),
                        _p(arr("plane_meas", np.float32, (-1, 4), z)), _p(arr("plane_world", np.float32, (-1, 12), z)),
                        _p(arr("plane_mask", np.uint8, -1, z)),
                        (C.c_double * 7)(*np.asarray(problems.get("plane_settings", np.zeros(7)), np.float64).tolist()))
    r = dict(Tcw=np.zeros((n, 16), np.float32), returns=np.zeros(n, np.int32), rounds=np.zeros(n, np.int32),
             iterations=np.zeros(n, np.int32), trials=np.zeros(n, np.int32), diag=np.zeros((n, 8), np.int32),
             point_outlier=np.zeros(nP, np.uint8), line_outlier=np.zeros(nL, np.uint8), plane_outlier=np.zeros(nS, np.uint8),
             par_plane_outlier=np.zeros(nS, np.uint8), ver_plane_outlier=np.zeros(nS, np.uint8))
    out = PoseOptOut(*[_p(r[k]) for k in POSE_OPT_OUT_FIELDS])
    return P, out, r, keep


def pose_opt_host(problems):
    """Optimizer::PoseOptimization of every frame on the host (drfe_pose_opt_host); problems and result as
    _pose_opt_pack"""
    P, out, r, _keep = _pose_opt_pack(problems)
    rc = load().drfe_pose_opt_host(C.byref(P), C.byref(out))
    if rc != 0:
        raise DrfeError(f"drfe_pose_opt_host failed ({rc})")
    return r


TRANSOPT_DEVICE_FROM = 64                            # DRFE_TRANSOPT_DEVICE_FROM


def trans_opt_host(problems):
    """Optimizer::TranslationOptimization of every frame on the host (drfe_trans_opt_host); problems and
    result as _pose_opt_pack: the map geometry stays in world coordinates, the entry rotates it"""
    P, out, r, _keep = _pose_opt_pack(problems)
    rc = load().drfe_trans_opt_host(C.byref(P), C.byref(out))
    if rc != 0:
        raise DrfeError(f"drfe_trans_opt_host failed ({rc})")
    return r


def trans_opt_plane_error(kind, meas, world, Tcw):
    """trans_opt_core.h's computeError of one translation-only plane edge (kind 3 matched, 4 parallel, 5 vertical): the world plane
    rotated by the float R_cw of Tcw, then the error under Tcw's translation: e [3]"""
    meas, world, Tcw = (np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in (meas, world, Tcw))
    e = np.zeros(3, np.float64)
    if load().drfe_debug_trans_opt_plane_error(int(kind), _p(meas), _p(world), _p(Tcw), _p(e)) != 0:
        raise DrfeError("drfe_debug_trans_opt_plane_error failed")
    return e


def _sim3_opt_pack(problems):
    """Packs a set of OptimizeSim3 problems (dict: S12 [n, 8] (quaternion x y z w, t, s), K1 / K2 [n, 4] (fx, fy, cx, cy), R1w / R2w
    [n, 9], t1w / t2w [n, 3], th2 [n], fix_scale [n], match_offsets [n + 1]; per kept match index [M], P3D1w / P3D2w [M, 3], obs1 /
    obs2 [M, 2], inv_sigma2_1 / inv_sigma2_2 [M]) into drfe_sim3_opt_problems and allocates the outputs: (problems record, out
    record, the outputs as a dict, the arrays to keep alive).  The outputs: per problem S12 [8], T12 [16], Scw [16], returns, n_bad,
    iterations [2], trials [2], diag [8] (SIM3_OPT_DIAG names the first seven); per match the outlier byte."""
    keep = {}
    kinds = dict(S12=(np.float64, (-1, 8)), K1=(np.float32, (-1, 4)), K2=(np.float32, (-1, 4)), R1w=(np.float32, (-1, 9)),
                 t1w=(np.float32, (-1, 3)), R2w=(np.float32, (-1, 9)), t2w=(np.float32, (-1, 3)), th2=(np.float32, (-1,)),
                 fix_scale=(np.uint8, (-1,)), match_offsets=(np.int32, (-1,)), index=(np.int32, (-1,)),
                 P3D1w=(np.float32, (-1, 3)), P3D2w=(np.float32, (-1, 3)), obs1=(np.float32, (-1, 2)), obs2=(np.float32, (-1, 2)),
                 inv_sigma2_1=(np.float32, (-1,)), inv_sigma2_2=(np.float32, (-1,)))
    for k in SIM3_OPT_IN_FIELDS:
        dt, shape = kinds[k]
        v = np.asarray(problems.get(k, np.zeros(0)), dt)
        keep[k] = np.ascontiguousarray(v.reshape(shape) if v.size else np.zeros((0,) + shape[1:], dt))
    off = keep["match_offsets"]
    n = len(off) - 1
    nM = max(int(off[-1]), 0) if len(off) else 0
    P = Sim3OptProblems(n, 0, *[_p(keep[k]) for k in SIM3_OPT_IN_FIELDS])
    r = dict(S12=np.zeros((n, 8), np.float64), T12=np.zeros((n, 16), np.float32), Scw=np.zeros((n, 16), np.float32),
             returns=np.zeros(n, np.int32), n_bad=np.zeros(n, np.int32), iterations=np.zeros((n, 2), np.int32),
             trials=np.zeros((n, 2), np.int32), diag=np.zeros((n, 8), np.int32), outlier=np.zeros(nM, np.uint8))
    out = Sim3OptOut(*[_p(r[k]) for k in SIM3_OPT_OUT_FIELDS])
    return P, out, r, keep


def sim3_opt_host(problems):
    """Optimizer::OptimizeSim3 of every problem on the host (drfe_sim3_opt_host); problems and result as
    _sim3_opt_pack"""
    P, out, r, _keep = _sim3_opt_pack(problems)
    rc = load().drfe_sim3_opt_host(C.byref(P), C.byref(out))
    if rc != 0:
        raise DrfeError(f"drfe_sim3_opt_host failed ({rc})")
    return r


def sim3_opt_ldlt(A, b):
    """the 7x7 form of pose_opt_core.h's Eigen::LDLT of the symmetric A (its lower triangle) and solve of A x = b: (isPositive, x)"""
    A = np.ascontiguousarray(np.asarray(A, np.float64).reshape(7, 7))
    b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(7))
    x, pos = np.zeros(7, np.float64), np.zeros(1, np.int32)
    if load().drfe_debug_sim3_opt_ldlt(_p(A), _p(b), _p(x), _p(pos)) != 0:
        raise DrfeError("drfe_debug_sim3_opt_ldlt failed")
    return bool(pos[0]), x


def sim3_opt_step(S12, x, b, lam, fix_scale, read_before=False):
    """sim3_opt_core.h's VertexSim3Expmap::oplusImpl of x [7] on S12 [8] and Levenberg's computeScale over (x, b, lambda), read after
    the update as g2o does or, with read_before, before oplusImpl wrote x[6] = 0 for a fixed scale: (S12 after the step, scale)"""
    S12 = np.ascontiguousarray(np.asarray(S12, np.float64).reshape(8))
    xbl = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).reshape(7), np.asarray(b, np.float64).reshape(7),
                                               np.asarray([lam], np.float64)]))
    out, scale = np.zeros(8, np.float64), np.zeros(1, np.float64)
    if load().drfe_debug_sim3_opt_step(_p(S12), _p(xbl), int(bool(fix_scale)), int(bool(read_before)), _p(out), _p(scale)) != 0:
        raise DrfeError("drfe_debug_sim3_opt_step failed")
    return out, float(scale[0])


def cr_cube(x):
    """cr_cube.h's correctly rounded x^3: (values [n], certified [n])"""
    x = np.ascontiguousarray(np.asarray(x, np.float64).reshape(-1))
    out, ok = np.zeros(len(x), np.float64), np.zeros(len(x), np.uint8)
    if load().drfe_debug_cr_cube(_p(x), len(x), _p(out), _p(ok)) != 0:
        raise DrfeError("drfe_debug_cr_cube failed")
    return out, ok.astype(bool)


def pose_opt_plane_error(kind, meas, world, Tcw):
    """pose_opt_core.h's computeError of one plane edge (kind 3 matched, 4 parallel, 5 vertical) under the float pose Tcw: e [3]"""
    meas, world, Tcw = (np.ascontiguousarray(np.asarray(v, np.float32).reshape(-1)) for v in (meas, world, Tcw))
    e = np.zeros(3, np.float64)
    if load().drfe_debug_pose_opt_plane_error(int(kind), _p(meas), _p(world), _p(Tcw), _p(e)) != 0:
        raise DrfeError("drfe_debug_pose_opt_plane_error failed")
    return e


def pose_opt_ldlt(A, b):
    """pose_opt_core.h's Eigen::LDLT of the symmetric 6x6 A (its lower triangle) and solve of A x = b: (isPositive, x)"""
    A = np.ascontiguousarray(np.asarray(A, np.float64).reshape(6, 6))
    b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(6))
    x, pos = np.zeros(6, np.float64), np.zeros(1, np.int32)
    if load().drfe_debug_pose_opt_ldlt(_p(A), _p(b), _p(x), _p(pos)) != 0:
        raise DrfeError("drfe_debug_pose_opt_ldlt failed")
    return bool(pos[0]), x


def _init_pack(problems):
    """Packs a problem set (dict: K [n, 9] (mK row-major), sigma [n], max_iterations [n], seed [n], key1_offsets [n + 1],
    key2_offsets [n + 1], keys1 [M1, 2], keys2 [M2, 2], matches12 [M1]) into drfe_init_problems and allocates the outputs:
    (problems record, out record, the outputs as a dict, the arrays to keep alive).  The outputs: the fields of drfe_init_out
    under their names, plus per solver row0, words, mask0 (N is filled by the call, so words and mask0 are computed here from
    matches12).  Solver s's rows are row0[s] + h, its mask words mask0[s] + h * words[s] + (i // 64), its motion hypothesis m
    entry [s, m] of the motion_* arrays and the slice [8 * key1_offsets[s] + m * nKeys1, + nKeys1) of motion_vbGood / motion_vP3D
    (init_table slices them)."""
    keep = []

    def arr(key, dt, shape=-1):
        v = np.ascontiguousarray(np.asarray(problems[key], dt).reshape(shape))
        keep.append(v)
        return v
    o1, o2 = arr("key1_offsets", np.int32), arr("key2_offsets", np.int32)
    n = len(o1) - 1
    maxit, m12 = arr("max_iterations", np.int32), arr("matches12", np.int32)
    P = InitProblems(n, 0, _p(arr("K", np.float32, (-1, 9))), _p(arr("sigma", np.float32)), _p(maxit), _p(arr("seed", np.uint32)),
                     _p(o1), _p(o2), _p(arr("keys1", np.float32, (-1, 2))), _p(arr("keys2", np.float32, (-1, 2))), _p(m12))
    cap = np.clip(maxit.astype(np.int64), 0, None)
    N = np.array([int((m12[max(int(o1[s]), 0):max(int(o1[s + 1]), 0)] >= 0).sum()) for s in range(n)], np.int64)
    words = (N + 63) // 64
    row0 = np.concatenate([[0], np.cumsum(cap)])
    mask0 = np.concatenate([[0], np.cumsum(cap * words)])
    rows, W, M1 = int(row0[-1]), int(mask0[-1]), max(int(o1[-1]), 0) if n else 0
    i32, f32 = np.int32, np.float32
    r = dict(N=np.zeros(n, i32), iterations=np.zeros(n, i32), hypotheses=np.zeros(n, i32), SH=np.zeros(n, f32), SF=np.zeros(n, f32),
             RH=np.zeros(n, f32), branch=np.zeros(n, i32), motions=np.zeros(n, i32), ok=np.zeros(n, i32), flags=np.zeros(n, i32),
             R21=np.zeros((n, 9), f32), t21=np.zeros((n, 3), f32), vP3D=np.zeros((M1, 3), f32), vbTriangulated=np.zeros(M1, np.uint8),
             sample=np.zeros((rows, 8), i32), H21=np.zeros((rows, 9), f32), F21=np.zeros((rows, 9), f32),
             score_h=np.zeros(rows, f32), score_f=np.zeros(rows, f32), best_h=np.zeros(rows, i32), best_f=np.zeros(rows, i32),
             mask_h=np.zeros(W, np.uint64), mask_f=np.zeros(W, np.uint64), motion_R=np.zeros((n, 8, 9), f32),
             motion_t=np.zeros((n, 8, 3), f32), motion_good=np.zeros((n, 8), i32), motion_cos=np.zeros((n, 8), f32),
             motion_parallax=np.zeros((n, 8), f32), motion_status=np.zeros((n, 8), i32), motion_vbGood=np.zeros(8 * M1, np.uint8),
             motion_vP3D=np.zeros((8 * M1, 3), f32))
    out = InitOut(*[_p(r[k]) for k in INIT_OUT_FIELDS])
    r.update(row0=row0[:-1], words=words, mask0=mask0[:-1], key1_offsets=o1.copy())
    return P, out, r, keep


def _init_call(fn, head, problems):
    """fn(*head, problems, out) over _init_pack's records: (return code, outputs)"""
    P, out, r, _keep = _init_pack(problems)
    rc = fn(*head, C.byref(P), C.byref(out), *([None] if head else []))
    return rc, r


def init_ransac_host(problems):
    """Initializer::Initialize of every solver on the host (drfe_init_ransac_host); problems and result as
    _init_pack"""
    rc, r = _init_call(load().drfe_init_ransac_host, (), problems)
    if rc != 0:
        raise DrfeError(f"drfe_init_ransac_host failed ({rc})")
    return r


def init_table(result, s):
    """Solver s of an init_ransac_* result: its scalars as Python numbers, R21 [9], t21 [3], vP3D [nKeys1, 3], vbTriangulated
    [nKeys1], its filled rows (sample, H21, F21, score_h, score_f, best_h, best_f, mask_h / mask_f [rows, words]) and its motion
    hypotheses (motion_R [m, 9], motion_t [m, 3], motion_good, motion_cos, motion_parallax, motion_status [m], motion_vbGood
    [m, nKeys1], motion_vP3D [m, nKeys1, 3])"""
    a, n, w = int(result["row0"][s]), int(result["hypotheses"][s]), int(result["words"][s])
    t = {k: result[k][a:a + n] for k in ("sample", "H21", "F21", "score_h", "score_f", "best_h", "best_f")}
    m0 = int(result["mask0"][s])
    for k in ("mask_h", "mask_f"):
        t[k] = result[k][m0:m0 + n * w].reshape(n, w)
    for k in ("N", "iterations", "hypotheses", "branch", "motions", "ok", "flags"):
        t[k] = int(result[k][s])
    for k in ("SH", "SF", "RH"):
        t[k] = result[k][s]
    k1, k2 = int(result["key1_offsets"][s]), int(result["key1_offsets"][s + 1])
    nk, nm = k2 - k1, t["motions"]
    t["R21"], t["t21"], t["vP3D"], t["vbTriangulated"] = result["R21"][s], result["t21"][s], result["vP3D"][k1:k2], result["vbTriangulated"][k1:k2]
    for k in ("motion_R", "motion_t", "motion_good", "motion_cos", "motion_parallax", "motion_status"):
        t[k] = result[k][s, :nm]
    t["motion_vbGood"] = result["motion_vbGood"][8 * k1:8 * k1 + nm * nk].reshape(nm, nk)
    t["motion_vP3D"] = result["motion_vP3D"][8 * k1:8 * k1 + nm * nk].reshape(nm, nk, 3)
    return t


def init_cos_keys(c):
    """init_core.h's order of CheckRT's accepted cosines: (keys uint32 [n], the cosine each key stands for [n])"""
    c = np.ascontiguousarray(c, np.float32)
    key, value = np.zeros(len(c), np.uint32), np.zeros(len(c), np.float32)
    if load().drfe_debug_init_cos_keys(_p(c), len(c), _p(key), _p(value)) != 0:
        raise DrfeError("drfe_debug_init_cos_keys failed")
    return key, value


def init_null_vectors(points):
    """init_core.h's float Jacobi SVD on samples of eight normalised matches [n, 8, 4] (x1 y1 x2 y2): vt.row(8) of ComputeH21's
    16x9 system and of ComputeF21's 8x9 system, [n, 9] each"""
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 8, 4)
    h, f = np.zeros((len(points), 9), np.float32), np.zeros((len(points), 9), np.float32)
    if load().drfe_debug_init_null_vectors(_p(points), len(points), _p(h), _p(f)) != 0:
        raise DrfeError("drfe_debug_init_null_vectors failed")
    return h, f


def init_check_rt(K, R, t, sigma, matches, ctx=None):
    """CheckRT of one motion hypothesis over matches [n, 4] (u1 v1 u2 v2), every one an inlier and match i's reference key i:
    dict(good, cos, parallax, status, vbGood [n], vP3D [n, 3]); with a Context through the device's CheckRT kernel"""
    K, R, t = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (K, R, t))
    assert K.size == 9 and R.size == 9 and t.size == 3
    m = np.ascontiguousarray(matches, np.float32).reshape(-1, 4)
    n = len(m)
    good, status = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cos, par = np.zeros(1, np.float32), np.zeros(1, np.float32)
    vb, X = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    L = ctx.L if ctx is not None else load()
    rc = L.drfe_debug_init_check_rt(ctx.h if ctx is not None else None, _p(K), _p(R), _p(t), float(sigma), _p(m), n, _p(good), _p(cos),
                                    _p(par), _p(status), _p(vb), _p(X))
    if ctx is not None:
        ctx._chk(rc, "drfe_debug_init_check_rt")
    elif rc != 0:
        raise DrfeError("drfe_debug_init_check_rt failed")
    return dict(good=int(good[0]), cos=cos[0], parallax=par[0], status=int(status[0]), vbGood=vb, vP3D=X)


def pnp_svd(A):
    """pnp_core.h's double Jacobi SVD of a row-major m x n matrix (n <= m <= 12): (w [n], ut [n, m], vt [n, n])"""
    A = np.ascontiguousarray(A, np.float64)
    m, n = A.shape
    w, ut, vt = np.zeros(n), np.zeros((n, m)), np.zeros((n, n))
    if load().drfe_debug_pnp_svd(_p(A), m, n, _p(w), _p(ut), _p(vt)) != 0:
        raise DrfeError("drfe_debug_pnp_svd failed")
    return w, ut, vt


def pnp_inliers(R, t, K, p2d, Xw, max_err, ctx=None):
    """pnp_core.h's CheckInliers under the double pose R [9], t [3]: bool [n]; with a Context through the device's sweep"""
    R, t = np.ascontiguousarray(R, np.float64).reshape(9), np.ascontiguousarray(t, np.float64).reshape(3)
    K = np.ascontiguousarray(K, np.float32).reshape(4)
    p2d, Xw = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2), np.ascontiguousarray(Xw, np.float32).reshape(-1, 3)
    me = np.ascontiguousarray(max_err, np.float32)
    out = np.zeros(len(me), np.uint8)
    if ctx is not None:
        ctx._chk(ctx.L.drfe_debug_pnp_inliers_device(ctx.h, _p(R), _p(t), _p(K), _p(p2d), _p(Xw), _p(me), len(me), _p(out)),
                 "drfe_debug_pnp_inliers_device")
    elif load().drfe_debug_pnp_inliers(_p(R), _p(t), _p(K), _p(p2d), _p(Xw), _p(me), len(me), _p(out)) != 0:
        raise DrfeError("drfe_debug_pnp_inliers failed")
    return out.astype(bool)


def sim3_atan2(y, x):
    """dr_slam_amd/csrc/cr_atan2.h's correctly rounded atan2 over float64 arrays (y >= 0): (values, certified)"""
    y = np.ascontiguousarray(y, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    out, ok = np.zeros_like(y), np.zeros(len(y), np.int32)
    if load().drfe_debug_sim3_atan2(_p(y), _p(x), len(y), _p(out), _p(ok)) != 0:
        raise DrfeError("drfe_debug_sim3_atan2 failed")
    return out, ok


def sim3_rand(seed, n):
    """the first n values of glibc's rand() after srand(seed), from dr_slam_amd/csrc/glibc_rand.h"""
    out = np.zeros(n, np.int32)
    if load().drfe_debug_sim3_rand(int(seed), n, _p(out)) != 0:
        raise DrfeError("drfe_debug_sim3_rand failed")
    return out


def sim3_horn(P1, P2, fix_scale, libm=False):
    """sim3_core.h's ComputeSim3 over samples P1, P2 [n, 3, 3] (one point per column): ([n, 37] = R12, t12, s12, T12, T21;
    certified [n]); libm: atan2, sin, cos from the host's libm"""
    P1 = np.ascontiguousarray(P1, np.float32).reshape(-1, 9)
    P2 = np.ascontiguousarray(P2, np.float32).reshape(-1, 9)
    out, ok = np.zeros((len(P1), 37), np.float32), np.zeros(len(P1), np.int32)
    if load().drfe_debug_sim3_horn(_p(P1), _p(P2), len(P1), int(fix_scale), int(libm), _p(out), _p(ok)) != 0:
        raise DrfeError("drfe_debug_sim3_horn failed")
    return out, ok


def manhattan_math(which, x):
    """drfe_asin (0), drfe_exp (1), drfe_tanf (2) of include/drfe_math.h over float64 inputs (drfe_tanf: rounded to float32)"""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    if L.drfe_debug_manhattan_math(which, _p(x), len(x), _p(out)) != 0:
        raise DrfeError("drfe_debug_manhattan_math failed")
    return out


def make_camera(fx, fy, cx, cy, bf, depth_map_factor, width, height) -> Camera:
    """Frame constants for the no-distortion path (bounds = image, reference src/Frame.cc:884-889).
    depth_map_factor is the yaml DepthMapFactor; the reference inverts it (src/Tracking.cc:144-148)."""
    inv = np.float32(1.0) if abs(depth_map_factor) < 1e-5 else np.float32(1.0) / np.float32(depth_map_factor)
    return Camera(fx, fy, cx, cy, bf, float(inv), 0.0, float(width), 0.0, float(height))


def lines_is_good(lines, depth_f32, K9, cx, cy, invfx, invfy, k_as_f64=False, seed=1):
    """Frame::isLineGood (host entry, no context / GPU needed): returns (mvDepthLine, mvLines3D[n,6], inliers, n_good).
    k_as_f64=False is the reference as shipped (CV_32F mK read as double -> nothing is accepted)."""
    L = load()
    kl = np.ascontiguousarray(lines, KEYLINE_DTYPE)
    d = np.ascontiguousarray(depth_f32, np.float32)
    K = np.ascontiguousarray(K9, np.float32).reshape(9)
    n = len(kl)
    dl = np.zeros(max(n, 1), np.float32)
    l3 = np.zeros((max(n, 1), 6), np.float64)
    ni = np.zeros(max(n, 1), np.int32)
    good = C.c_int()
    rc = L.drfe_lines_is_good(_p(kl), n, _p(d), d.shape[1], d.shape[0], d.shape[1], _p(K), int(bool(k_as_f64)),
                              C.c_float(cx), C.c_float(cy), C.c_float(invfx), C.c_float(invfy), int(seed), _p(dl), _p(l3),
                              _p(ni), C.byref(good))
    if rc != 0:
        raise RuntimeError(f"drfe_lines_is_good failed ({rc})")
    return dl[:n], l3[:n], ni[:n], good.value


def line3d_chunk_frames(cap):
    """frames of `cap` key lines that Context.lines_is_good_batch lifts at once; a larger call runs in chunks of that many"""
    return load().drfe_line3d_chunk_frames(int(cap))


def line3d_frames(lines, n_lines, depth, K9, cx, cy, invfx, invfy, k_as_f64=True, seeds=None, w=None):
    """drfe_line3d_frames and zeroed drfe_line3d_out over lines [F, cap] KEYLINE_DTYPE, n_lines [F], depth [F, h, stride]
    (float32 numpy, or a torch tensor on the device: depth_on_device) of images w wide (default: stride), seeds [F] or None:
    (frames, out, results (depth_line [F, cap] = -1, lines3d [F, cap, 6], n_inliers [F, cap], n_good [F]), keep-alive)"""
    kl = np.ascontiguousarray(lines, KEYLINE_DTYPE)
    F, cap = kl.shape
    nl = np.ascontiguousarray(n_lines, np.int32)
    on_device = not isinstance(depth, np.ndarray)
    d = depth.contiguous() if on_device else np.ascontiguousarray(depth, np.float32)
    assert len(nl) == F and d.shape[0] == F and len(d.shape) == 3 and (not on_device or "float32" in str(d.dtype))
    sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint32)
    h, stride = int(d.shape[1]), int(d.shape[2])
    fr = Line3dFrames(F, cap, _p(kl), _p(nl), C.c_void_p(d.data_ptr()) if on_device else _p(d), h * stride, stride,
                      stride if w is None else int(w), h, int(on_device), int(bool(k_as_f64)),
                      (C.c_float * 9)(*np.asarray(K9, np.float32).reshape(9).tolist()), float(cx), float(cy), float(invfx),
                      float(invfy), _p(sd))
    r = (np.full((F, cap), -1, np.float32), np.zeros((F, cap, 6), np.float64), np.zeros((F, cap), np.int32), np.zeros(F, np.int32))
    out = Line3dOut(*[_p(a) for a in r])
    return fr, out, r, (kl, nl, d, sd)


def _csr_i32(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists]) if len(lists) else [], np.int32)
    return off, flat


def kfdb_score(ids_a, vals_a, ids_b, vals_b):
    """TemplatedVocabulary::score of two BowVectors (L1), as float32 (drfe_kfdb_score)"""
    ia, ib = np.ascontiguousarray(ids_a, np.int32), np.ascontiguousarray(ids_b, np.int32)
    va, vb = np.ascontiguousarray(vals_a, np.float64), np.ascontiguousarray(vals_b, np.float64)
    out = np.zeros(1, np.float32)
    rc = load().drfe_kfdb_score(len(ia), _p(ia), _p(va), len(ib), _p(ib), _p(vb), _p(out))
    if rc != 0:
        raise DrfeError(f"drfe_kfdb_score failed ({rc})")
    return out[0]


class KeyFrameDatabase:
    """drfe_kfdb: KeyFrameDatabase with its loop and relocalisation queries.  ctx None = host-only; with a
    Context, mode "device" runs a call on its GPU and "batch" by the crossover.  A failing call raises DrfeError with .rc."""

    def __init__(self, ctx=None, scoring=KFDB_L1_NORM):
        self.L = load()
        self.ctx = ctx                                  # keeps the context alive
        h = C.c_void_p()
        rc = self.L.drfe_kfdb_create(ctx.h if ctx is not None else None, int(scoring), C.byref(h))
        if rc != 0:
            e = DrfeError(f"drfe_kfdb_create failed ({rc})")
            e.rc = rc
            raise e
        self.h = h

    def _chk(self, rc, what):
        if rc != 0:
            e = DrfeError(f"{what} failed ({rc}): {self.L.drfe_kfdb_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def close(self):
        if getattr(self, "h", None):
            self.L.drfe_kfdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def put(self, handle, word_ids, values):
        ids = np.ascontiguousarray(word_ids, np.int32)
        vals = np.ascontiguousarray(values, np.float64)
        assert ids.shape == vals.shape and ids.ndim == 1
        self._chk(self.L.drfe_kfdb_put(self.h, int(handle), len(ids), _p(ids), _p(vals)), "drfe_kfdb_put")

    def add(self, handle):
        self._chk(self.L.drfe_kfdb_add(self.h, int(handle)), "drfe_kfdb_add")

    def erase(self, handle):
        self._chk(self.L.drfe_kfdb_erase(self.h, int(handle)), "drfe_kfdb_erase")

    def remove(self, handle):
        self._chk(self.L.drfe_kfdb_remove(self.h, int(handle)), "drfe_kfdb_remove")

    def clear(self):
        self._chk(self.L.drfe_kfdb_clear(self.h), "drfe_kfdb_clear")

    def set_neighbours(self, handles, nbr):
        """nbr: one list of at most 10 handles per key frame (GetBestCovisibilityKeyFrames(10)); padded with -1 here"""
        hs = np.ascontiguousarray(handles, np.int32)
        tab = np.full((len(hs), KFDB_NEIGHBOURS), -1, np.int32)
        for i, row in enumerate(nbr):
            row = np.asarray(row, np.int32).reshape(-1)[:KFDB_NEIGHBOURS]
            tab[i, :len(row)] = row
        self._chk(self.L.drfe_kfdb_set_neighbours(self.h, len(hs), _p(hs), _p(tab)), "drfe_kfdb_set_neighbours")

    def size(self):
        out = np.zeros(2, np.int32)
        self._chk(self.L.drfe_kfdb_size(self.h, _p(out)), "drfe_kfdb_size")
        return int(out[0]), int(out[1])

    def stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_kfdb_stats(self.h, _p(st)), "drfe_kfdb_stats")
        return dict(zip(KFDB_STATS, (int(v) for v in st)))

    def _run(self, kind, Q, n, mode, capacity):
        if capacity is None:
            capacity = n * (self.size()[1] + n)
        r = {"cand_offsets": np.zeros(n + 1, np.int32), "candidates": np.zeros(max(1, capacity), np.int32),
             "record": np.zeros((n, 4), np.int32), "min_score": np.zeros(n, np.float32), "uninit_reads": np.zeros(n, np.int32)}
        out = KfdbOut(int(capacity), 0, *[_p(r[k]) for k in ("cand_offsets", "candidates", "record", "min_score", "uninit_reads")])
        fn = getattr(self.L, f"drfe_kfdb_{kind}_queries_{mode}")
        args = (self.h, C.byref(Q), C.byref(out)) + (() if mode == "host" else (None,))
        self._chk(fn(*args), f"drfe_kfdb_{kind}_queries_{mode}")
        off = r["cand_offsets"]
        r["candidates"] = [r["candidates"][off[k]:off[k + 1]].copy() for k in range(n)]
        return r

    def loop_queries(self, queries, mode="host", capacity=None):
        """DetectLoopCandidates of every query: dicts with handle, id, connected (handles) and either min_score or covisible
        (handles, GetVectorCovisibleKeyFrames order), and add_after (default False).  Returns candidates (one array of handles per
        query), min_score [n], record [n, 4] (listed, scored, kept, maxCommonWords)."""
        n = len(queries)
        explicit = [("min_score" in q) for q in queries]
        assert all(explicit) or not any(explicit), "either every query gives min_score or none does"
        handle = np.array([q["handle"] for q in queries], np.int32)
        ident = np.array([q["id"] for q in queries], np.int64)
        coff, conn = _csr_i32([q.get("connected", ()) for q in queries])
        voff, cov = _csr_i32([q.get("covisible", ()) for q in queries])
        ms = np.array([q["min_score"] for q in queries], np.float32) if n and explicit[0] else None
        after = np.array([1 if q.get("add_after") else 0 for q in queries], np.uint8)
        Q = KfdbLoopQueries(n, 0, _p(handle), _p(ident), _p(coff), _p(conn), _p(ms), _p(voff), _p(cov), _p(after))
        return self._run("loop", Q, n, mode, capacity)

    def reloc_queries(self, queries, mode="host", capacity=None):
        """DetectRelocalizationCandidates of every query (id, word_ids, values), as if run one after another.  Returns candidates,
        record [n, 4] and uninit_reads [n]."""
        n = len(queries)
        ident = np.array([q[0] for q in queries], np.int64)
        off, ids = _csr_i32([q[1] for q in queries])
        vals = np.ascontiguousarray(np.concatenate([np.asarray(q[2], np.float64).reshape(-1) for q in queries]) if n else [],
                                    np.float64)
        Q = KfdbRelocQueries(n, 0, _p(ident), _p(off), _p(ids), _p(vals))
        return self._run("reloc", Q, n, mode, capacity)


class LocalMap:
    """drfe_lmap: the part of the map graph Tracking::UpdateLocalMap reads, and that function for every frame
    of a call.  ctx None = host-only; with a Context, mode "device" runs a call on its GPU and "batch" by the crossover.  A failing
    call raises DrfeError with .rc."""

    def __init__(self, ctx=None):
        self.L = load()
        self.ctx = ctx                                  # keeps the context alive
        h = C.c_void_p()
        rc = self.L.drfe_lmap_create(ctx.h if ctx is not None else None, C.byref(h))
        if rc != 0:
            e = DrfeError(f"drfe_lmap_create failed ({rc})")
            e.rc = rc
            raise e
        self.h = h

    def _chk(self, rc, what):
        if rc != 0:
            e = DrfeError(f"{what} failed ({rc}): {self.L.drfe_lmap_last_error(self.h).decode()}")
            e.rc = rc
            raise e

    def close(self):
        if getattr(self, "h", None):
            self.L.drfe_lmap_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def limits():
        out = np.zeros(4, np.int32)
        rc = load().drfe_lmap_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_limits failed ({rc})")
        return dict(zip(LMAP_LIMITS, (int(v) for v in out)))

    def configure(self, scratch_bytes):
        self._chk(self.L.drfe_lmap_configure(self.h, int(scratch_bytes)), "drfe_lmap_configure")

    def set_keyframes(self, rows):
        """rows: dicts with handle, rank, and optionally bad, parent (-1), neighbours (at most 10 handles, padded with -1 here),
        children, points, lines (handles by keypoint index, -1 = null)"""
        n = len(rows)
        handle = np.array([r["handle"] for r in rows], np.int32)
        rank = np.array([r["rank"] for r in rows], np.uint64)
        bad = np.array([1 if r.get("bad") else 0 for r in rows], np.uint8)
        parent = np.array([r.get("parent", -1) for r in rows], np.int32)
        nbr = np.full((n, LMAP_NEIGHBOURS), -1, np.int32)
        for i, r in enumerate(rows):
            row = np.asarray(r.get("neighbours", ()), np.int32).reshape(-1)[:LMAP_NEIGHBOURS]
            nbr[i, :len(row)] = row
        coff, ch = _csr_i32([r.get("children", ()) for r in rows])
        poff, pts = _csr_i32([r.get("points", ()) for r in rows])
        loff, lns = _csr_i32([r.get("lines", ()) for r in rows])
        K = LmapKeyframes(n, 0, _p(handle), _p(rank), _p(bad), _p(parent), _p(nbr), _p(coff), _p(ch), _p(poff), _p(pts), _p(loff),
                          _p(lns))
        self._chk(self.L.drfe_lmap_set_keyframes(self.h, C.byref(K)), "drfe_lmap_set_keyframes")

    def set_points(self, rows):
        """rows: dicts with handle, and optionally bad and obs (the key-frame handles of GetObservations())"""
        handle = np.array([r["handle"] for r in rows], np.int32)
        bad = np.array([1 if r.get("bad") else 0 for r in rows], np.uint8)
        off, obs = _csr_i32([r.get("obs", ()) for r in rows])
        self._chk(self.L.drfe_lmap_set_points(self.h, len(rows), _p(handle), _p(bad), _p(off), _p(obs)), "drfe_lmap_set_points")

    def set_lines(self, handles, bad=None):
        hs = np.ascontiguousarray(handles, np.int32)
        b = np.zeros(len(hs), np.uint8) if bad is None else np.ascontiguousarray(bad, np.uint8)
        self._chk(self.L.drfe_lmap_set_lines(self.h, len(hs), _p(hs), _p(b)), "drfe_lmap_set_lines")

    def set_bad(self, kind, handles, flags):
        hs = np.ascontiguousarray(handles, np.int32)
        b = np.ascontiguousarray(flags, np.uint8)
        assert hs.shape == b.shape
        self._chk(self.L.drfe_lmap_set_bad(self.h, int(kind), len(hs), _p(hs), _p(b)), "drfe_lmap_set_bad")

    def remove(self, kind, handle):
        self._chk(self.L.drfe_lmap_remove(self.h, int(kind), int(handle)), "drfe_lmap_remove")

    def size(self):
        out = np.zeros(3, np.int32)
        self._chk(self.L.drfe_lmap_size(self.h, _p(out)), "drfe_lmap_size")
        return int(out[0]), int(out[1]), int(out[2])

    def stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_stats(self.h, _p(st)), "drfe_lmap_stats")
        return dict(zip(LMAP_STATS, (int(v) for v in st)))

    def update(self, queries, mode="batch", capacity=None):
        """UpdateLocalMap of every frame: dicts with frame_id, points (handles by keypoint index, -1 = null) and optionally lines
        and prev_kfs.  Returns a dict: kfs, mps, mp_in_frame, mls, ml_in_frame, nulled (one array per query), ref_kf [n] and
        record [n, 4].  capacity: (kf, mp, ml, nulled), default the bounds of drfe_lmap_size."""
        n = len(queries)
        ident = np.array([q["frame_id"] for q in queries], np.int64)
        poff, pts = _csr_i32([q.get("points", ()) for q in queries])
        has_l = any("lines" in q for q in queries)
        has_v = any("prev_kfs" in q for q in queries)
        loff, lns = _csr_i32([q.get("lines", ()) for q in queries]) if has_l else (None, None)
        voff, prev = _csr_i32([q.get("prev_kfs", ()) for q in queries]) if has_v else (None, None)
        if capacity is None:
            nk, npt, nl = self.size()
            capacity = (n * nk + (len(prev) if has_v else 0), n * npt, n * nl, len(pts))
        ckf, cmp_, cml, cnu = (int(c) for c in capacity)
        r = {"kf_offsets": np.zeros(n + 1, np.int32), "kfs": np.zeros(max(1, ckf), np.int32), "ref_kf": np.zeros(n, np.int32),
             "mp_offsets": np.zeros(n + 1, np.int32), "mps": np.zeros(max(1, cmp_), np.int32),
             "mp_in_frame": np.zeros(max(1, cmp_), np.uint8), "ml_offsets": np.zeros(n + 1, np.int32),
             "mls": np.zeros(max(1, cml), np.int32), "ml_in_frame": np.zeros(max(1, cml), np.uint8),
             "nulled_offsets": np.zeros(n + 1, np.int32), "nulled": np.zeros(max(1, cnu), np.int32),
             "record": np.zeros((n, 4), np.int32)}
        Q = LmapQueries(n, 0, _p(ident), _p(poff), _p(pts), _p(loff), _p(lns), _p(voff), _p(prev))
        out = LmapOut(ckf, cmp_, cml, cnu, *[_p(r[k]) for k in LMAP_OUT_FIELDS])
        fn = getattr(self.L, f"drfe_lmap_update_{mode}")
        args = (self.h, C.byref(Q), C.byref(out)) + (() if mode == "host" else (None,))
        self._chk(fn(*args), f"drfe_lmap_update_{mode}")
        res = {"ref_kf": r["ref_kf"], "record": r["record"]}
        for name, off in (("kfs", "kf_offsets"), ("mps", "mp_offsets"), ("mp_in_frame", "mp_offsets"), ("mls", "ml_offsets"),
                          ("ml_in_frame", "ml_offsets"), ("nulled", "nulled_offsets")):
            o = r[off]
            res[name] = [r[name][o[k]:o[k + 1]].copy() for k in range(n)]
        return res

    # ---- KeyFrame::UpdateConnections on the store ----

    @staticmethod
    def connect_limits():
        out = np.zeros(4, np.int32)
        rc = load().drfe_lmap_connect_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_connect_limits failed ({rc})")
        return dict(zip(LMAP_CONNECT_LIMITS, (int(v) for v in out)))

    def connect_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_connect_stats(self.h, _p(st)), "drfe_lmap_connect_stats")
        return dict(zip(LMAP_CONNECT_STATS, (int(v) for v in st)))

    def set_connections(self, rows):
        """rows: dicts with handle, and optionally first (mbFirstConnection && mnId != 0), weights and ordered: lists of
        (key-frame handle, weight) pairs - mConnectedKeyFrameWeights in any order, the ordered list in the reference's order"""
        handle = np.array([r["handle"] for r in rows], np.int32)
        first = np.array([1 if r.get("first") else 0 for r in rows], np.uint8)
        woff, wkf = _csr_i32([[p[0] for p in r.get("weights", ())] for r in rows])
        _, ww = _csr_i32([[p[1] for p in r.get("weights", ())] for r in rows])
        ooff, okf = _csr_i32([[p[0] for p in r.get("ordered", ())] for r in rows])
        _, ow = _csr_i32([[p[1] for p in r.get("ordered", ())] for r in rows])
        K = LmapConnections(len(rows), 0, _p(handle), _p(first), _p(woff), _p(wkf), _p(ww), _p(ooff), _p(okf), _p(ow))
        self._chk(self.L.drfe_lmap_set_connections(self.h, C.byref(K)), "drfe_lmap_set_connections")

    @staticmethod
    def _conn_rows(n_rows, cw, co):
        r = {"weight_offsets": np.zeros(n_rows + 1, np.int32), "weight_kfs": np.zeros(max(1, cw), np.int32),
             "weight_w": np.zeros(max(1, cw), np.int32), "ordered_offsets": np.zeros(n_rows + 1, np.int32),
             "ordered_kfs": np.zeros(max(1, co), np.int32), "ordered_w": np.zeros(max(1, co), np.int32),
             "parent": np.zeros(max(1, n_rows), np.int32), "first_connection": np.zeros(max(1, n_rows), np.uint8)}
        return r, LmapConnRows(cw, co, *[_p(r[k]) for k in LMAP_CONN_ROWS_FIELDS])

    @staticmethod
    def _conn_unpack(r, n):
        out = {"parent": r["parent"][:n].copy(), "first": r["first_connection"][:n].copy()}
        for name, off, kf, w in (("weights", "weight_offsets", "weight_kfs", "weight_w"),
                                 ("ordered", "ordered_offsets", "ordered_kfs", "ordered_w")):
            o = r[off]
            out[name] = [np.stack([r[kf][o[k]:o[k + 1]], r[w][o[k]:o[k + 1]]], axis=1) for k in range(n)]
        return out

    def get_connections(self, handles):
        """the stored state of the named key frames: dict of parent [n], first [n], weights and ordered (one [m, 2] array of
        (handle, weight) per key frame; weights in ascending rank) and children (one array per key frame, ascending rank)"""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        cap = 1 << 12
        while True:
            r, rows = self._conn_rows(n, cap, cap)
            coff, ch = np.zeros(n + 1, np.int32), np.zeros(cap, np.int32)
            rc = self.L.drfe_lmap_get_connections(self.h, n, _p(hs), C.byref(rows), cap, _p(coff), _p(ch))
            if rc != ERR_CAPACITY:
                break
            cap *= 4
        self._chk(rc, "drfe_lmap_get_connections")
        out = self._conn_unpack(r, n)
        out["children"] = [ch[coff[k]:coff[k + 1]].copy() for k in range(n)]
        return out

    def connect(self, handles, mode="batch", capacity=None):
        """UpdateConnections of the named key frames, one after another in that order.  Returns a dict: counter (one [m, 2] array of
        (handle, votes) per called key frame), record [n, 4], new_parent [n]; touched [t] and, per touched key frame, weights,
        ordered, parent, first, flags.  capacity: (counter, touched, weights, ordered); default: the documented bounds for the
        first two and arrays grown until the call fits for the others (a call that does not fit changes nothing)."""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        fn = getattr(self.L, f"drfe_lmap_connect_{mode}")
        grow = capacity is None
        if grow:
            nk = self.size()[0]
            capacity = (n * max(nk - 1, 0), nk, 1 << 14, 1 << 14)
        cc, ct, cw, co = (int(c) for c in capacity)
        while True:
            r, rows = self._conn_rows(ct, cw, co)
            c = {"counter_offsets": np.zeros(n + 1, np.int32), "counter_kfs": np.zeros(max(1, cc), np.int32),
                 "counter_votes": np.zeros(max(1, cc), np.int32), "record": np.zeros((n, 4), np.int32),
                 "new_parent": np.zeros(max(1, n), np.int32), "n_touched": np.zeros(1, np.int32),
                 "touched": np.zeros(max(1, ct), np.int32), "flags": np.zeros(max(1, ct), np.uint8)}
            out = LmapConnectOut(cc, ct, _p(c["counter_offsets"]), _p(c["counter_kfs"]), _p(c["counter_votes"]), _p(c["record"]),
                                 _p(c["new_parent"]), _p(c["n_touched"]), _p(c["touched"]), rows, _p(c["flags"]))
            args = (self.h, n, _p(hs), C.byref(out)) + (() if mode == "host" else (None,))
            rc = fn(*args)
            if not (grow and rc == ERR_CAPACITY and cw < nk * nk):       # nk x nk always suffices: what remains is the scratch budget
                break
            cw, co = cw * 8, co * 8
        self._chk(rc, f"drfe_lmap_connect_{mode}")
        nt = int(c["n_touched"][0])
        res = self._conn_unpack(r, nt)
        o = c["counter_offsets"]
        res.update(counter=[np.stack([c["counter_kfs"][o[k]:o[k + 1]], c["counter_votes"][o[k]:o[k + 1]]], axis=1) for k in range(n)],
                   record=c["record"], new_parent=c["new_parent"][:n].copy(), touched=c["touched"][:nt].copy(),
                   flags=c["flags"][:nt].copy())
        return res

    # ---- LoopClosing::CorrectLoop's Sim3 propagation on the store ----

    @staticmethod
    def correct_limits():
        out = np.zeros(4, np.int32)
        rc = load().drfe_lmap_correct_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_correct_limits failed ({rc})")
        return dict(zip(LMAP_CORRECT_LIMITS, (int(v) for v in out)))

    def correct_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_correct_stats(self.h, _p(st)), "drfe_lmap_correct_stats")
        return dict(zip(LMAP_CORRECT_STATS, (int(v) for v in st)))

    def correct_scratch(self, handles):
        """bytes of device scratch a correct call of these key frames takes: (as one chunk, at least, shared by every chunk)"""
        hs = np.ascontiguousarray(handles, np.int32)
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_correct_scratch(self.h, len(hs), _p(hs), _p(out)), "drfe_lmap_correct_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def set_scales(self, scale_factors):
        sf = np.ascontiguousarray(scale_factors, np.float32)
        self._chk(self.L.drfe_lmap_set_scales(self.h, len(sf), _p(sf)), "drfe_lmap_set_scales")

    def get_scales(self):
        n = np.zeros(1, np.int32)
        sf = np.zeros(64, np.float32)
        rc = self.L.drfe_lmap_get_scales(self.h, len(sf), _p(n), _p(sf))
        if rc == ERR_CAPACITY:
            sf = np.zeros(int(n[0]), np.float32)
            rc = self.L.drfe_lmap_get_scales(self.h, len(sf), _p(n), _p(sf))
        self._chk(rc, "drfe_lmap_get_scales")
        return sf[:int(n[0])].copy()

    def set_poses(self, handles, Tcw):
        """Tcw [n, 4, 4] float32, what SetPose received"""
        hs = np.ascontiguousarray(handles, np.int32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(len(hs), 16)
        self._chk(self.L.drfe_lmap_set_poses(self.h, len(hs), _p(hs), _p(T)), "drfe_lmap_set_poses")

    def get_poses(self, handles):
        """dict of Tcw [n, 4, 4], Ow [n, 3] and Twc [n, 4, 4] as SetPose derives them"""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        T, O, W = np.zeros((n, 4, 4), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 4, 4), np.float32)
        self._chk(self.L.drfe_lmap_get_poses(self.h, n, _p(hs), _p(T), _p(O), _p(W)), "drfe_lmap_get_poses")
        return {"Tcw": T, "Ow": O, "Twc": W}

    def set_point_geometry(self, rows):
        """rows: dicts with handle, world (3 floats), ref_kf, and optionally ref_level (0), corrected_by (0), corrected_ref (0)"""
        n = len(rows)
        handle = np.array([r["handle"] for r in rows], np.int32)
        world = np.array([r["world"] for r in rows], np.float32).reshape(n, 3)
        ref = np.array([r["ref_kf"] for r in rows], np.int32)
        level = np.array([r.get("ref_level", 0) for r in rows], np.int32)
        by = np.array([r.get("corrected_by", 0) for r in rows], np.int32)
        byref = np.array([r.get("corrected_ref", 0) for r in rows], np.int32)
        G = LmapPointGeometry(n, 0, _p(handle), _p(world), _p(ref), _p(level), _p(by), _p(byref))
        self._chk(self.L.drfe_lmap_set_point_geometry(self.h, C.byref(G)), "drfe_lmap_set_point_geometry")

    def get_point_geometry(self, handles):
        """dict of world [n, 3], ref_kf, ref_level, corrected_by, corrected_ref [n]"""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        r = {"world": np.zeros((n, 3), np.float32), "ref_kf": np.zeros(n, np.int32), "ref_level": np.zeros(n, np.int32),
             "corrected_by": np.zeros(n, np.int32), "corrected_ref": np.zeros(n, np.int32)}
        self._chk(self.L.drfe_lmap_get_point_geometry(self.h, n, _p(hs), *[_p(v) for v in r.values()]),
                  "drfe_lmap_get_point_geometry")
        return r

    def correct(self, cur, Scw, handles, mode="batch", capacity=None):
        """CorrectLoop's propagation (src/LoopClosing.cc:480-562) for the current key frame `cur`, Scw = (qx, qy, qz, qw, tx, ty, tz,
        s) and the connected key frames `handles` (cur among them, any order).  Returns a dict: per called key frame, in the
        caller's order, walk_pos [n], corrected [n, 8], non_corrected [n, 8], Tiw [n, 4, 4]; per moved point, in walk order, points,
        claimed_by, world [m, 3], normal [m, 3], max_distance, min_distance, status.  capacity: moved points, default the total
        length of the called match rows (a call that does not fit changes nothing)."""
        hs = np.ascontiguousarray(handles, np.int32)
        S = np.ascontiguousarray(Scw, np.float64).reshape(8)
        n = len(hs)
        cap = 1 << 12 if capacity is None else int(capacity)
        fn = getattr(self.L, f"drfe_lmap_correct_{mode}")
        while True:
            m = max(1, cap)
            r = {"walk_pos": np.zeros(max(1, n), np.int32), "corrected": np.zeros((max(1, n), 8), np.float64),
                 "non_corrected": np.zeros((max(1, n), 8), np.float64), "Tiw": np.zeros((max(1, n), 4, 4), np.float32),
                 "n_points": np.zeros(1, np.int32), "points": np.zeros(m, np.int32), "claimed_by": np.zeros(m, np.int32),
                 "world": np.zeros((m, 3), np.float32), "normal": np.zeros((m, 3), np.float32),
                 "max_distance": np.zeros(m, np.float32), "min_distance": np.zeros(m, np.float32), "status": np.zeros(m, np.uint8)}
            out = LmapCorrectOut(cap, 0, *[_p(r[k]) for k in LMAP_CORRECT_OUT_FIELDS])
            args = (self.h, int(cur), _p(S), n, _p(hs), C.byref(out)) + (() if mode == "host" else (None,))
            rc = fn(*args)
            if not (capacity is None and rc == ERR_CAPACITY and cap < (1 << 28)
                    and b"points_capacity" in self.L.drfe_lmap_last_error(self.h)):
                break
            cap *= 8
        self._chk(rc, f"drfe_lmap_correct_{mode}")
        m = int(r["n_points"][0])
        res = {k: r[k][:n].copy() for k in ("walk_pos", "corrected", "non_corrected", "Tiw")}
        res.update({k: r[k][:m].copy() for k in LMAP_CORRECT_OUT_FIELDS[5:]})
        return res

    # ---- LocalMapping::KeyFrameCulling with KeyFrame::SetBadFlag on the store ----

    @staticmethod
    def cull_limits():
        out = np.zeros(4, np.int32)
        rc = load().drfe_lmap_cull_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_cull_limits failed ({rc})")
        return dict(zip(LMAP_CULL_LIMITS, (int(v) for v in out)))

    def cull_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_cull_stats(self.h, _p(st)), "drfe_lmap_cull_stats")
        return dict(zip(LMAP_CULL_STATS, (int(v) for v in st)))

    def upload_bytes(self):
        """host-to-device bytes since the store was made: dict of rows, graph, geometry, attributes, gba"""
        out = np.zeros(5, np.int64)
        self._chk(self.L.drfe_lmap_upload_bytes(self.h, _p(out)), "drfe_lmap_upload_bytes")
        return dict(zip(("rows", "graph", "geometry", "attributes", "gba"), (int(v) for v in out)))

    # ---- LocalMapping::MapPointCulling and MapLineCulling on the store ----

    @staticmethod
    def recent_cull_limits():
        out = np.zeros(6, np.int32)
        rc = load().drfe_lmap_recent_cull_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_recent_cull_limits failed ({rc})")
        return dict(zip(LMAP_RECENT_LIMITS, (int(v) for v in out)))

    def recent_cull_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_recent_cull_stats(self.h, _p(st)), "drfe_lmap_recent_cull_stats")
        return dict(zip(LMAP_RECENT_STATS, (int(v) for v in st)))

    def recent_upload_bytes(self):
        """host-to-device bytes of the recent-list block since the store was made"""
        out = np.zeros(1, np.int64)
        self._chk(self.L.drfe_lmap_recent_upload_bytes(self.h, _p(out)), "drfe_lmap_recent_upload_bytes")
        return int(out[0])

    def recent_cull_scratch(self, n_entries):
        """bytes of device scratch a recent_cull call of n_entries takes: (as one chunk, at least, shared by every chunk)"""
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_recent_cull_scratch(self.h, int(n_entries), _p(out)), "drfe_lmap_recent_cull_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def set_recent_attributes(self, points=(), lines=()):
        """points: dicts with handle, found, visible, first_kf.  lines: the same plus n_obs, obs (key-frame handles in the
        caller's order) and obs_index parallel to them."""
        ph = np.array([r["handle"] for r in points], np.int32)
        pf = np.array([r["found"] for r in points], np.int32)
        pv = np.array([r["visible"] for r in points], np.int32)
        p1 = np.array([r["first_kf"] for r in points], np.int64)
        lh = np.array([r["handle"] for r in lines], np.int32)
        lf = np.array([r["found"] for r in lines], np.int32)
        lv = np.array([r["visible"] for r in lines], np.int32)
        l1 = np.array([r["first_kf"] for r in lines], np.int64)
        ln = np.array([r["n_obs"] for r in lines], np.int32)
        ooff, obs = _csr_i32([r.get("obs", ()) for r in lines])
        ioff, idx = _csr_i32([r.get("obs_index", ()) for r in lines])
        if not np.array_equal(ooff, ioff):
            raise ValueError("obs and obs_index of a line must have one length")
        A = LmapRecentAttributes(len(ph), len(lh), _p(ph), _p(pf), _p(pv), _p(p1), _p(lh), _p(lf), _p(lv), _p(l1), _p(ln), _p(ooff),
                                 _p(obs), _p(idx))
        self._chk(self.L.drfe_lmap_set_recent_attributes(self.h, C.byref(A)), "drfe_lmap_set_recent_attributes")

    def get_recent_attributes(self, point_handles=(), line_handles=()):
        """the stored state: dict of points (dicts with handle, found, visible, first_kf) and lines (the same plus n_obs, obs,
        obs_index)"""
        ph = np.ascontiguousarray(point_handles, np.int32)
        lh = np.ascontiguousarray(line_handles, np.int32)
        npt, nl = len(ph), len(lh)
        cap = 1 << 12
        while True:
            r = {"pf": np.zeros(max(1, npt), np.int32), "pv": np.zeros(max(1, npt), np.int32), "p1": np.zeros(max(1, npt), np.int64),
                 "lf": np.zeros(max(1, nl), np.int32), "lv": np.zeros(max(1, nl), np.int32), "l1": np.zeros(max(1, nl), np.int64),
                 "ln": np.zeros(max(1, nl), np.int32), "off": np.zeros(nl + 1, np.int32), "obs": np.zeros(cap, np.int32),
                 "idx": np.zeros(cap, np.int32)}
            O = LmapRecentAttributesOut(npt, nl, cap, _p(ph), _p(r["pf"]), _p(r["pv"]), _p(r["p1"]), _p(lh), _p(r["lf"]), _p(r["lv"]),
                                        _p(r["l1"]), _p(r["ln"]), _p(r["off"]), _p(r["obs"]), _p(r["idx"]))
            rc = self.L.drfe_lmap_get_recent_attributes(self.h, C.byref(O))
            if rc != ERR_CAPACITY or cap >= (1 << 28):
                break
            cap *= 8
        self._chk(rc, "drfe_lmap_get_recent_attributes")
        o = r["off"]
        return {"points": [{"handle": int(ph[i]), "found": int(r["pf"][i]), "visible": int(r["pv"][i]), "first_kf": int(r["p1"][i])}
                           for i in range(npt)],
                "lines": [{"handle": int(lh[i]), "found": int(r["lf"][i]), "visible": int(r["lv"][i]), "first_kf": int(r["l1"][i]),
                           "n_obs": int(r["ln"][i]), "obs": r["obs"][o[i]:o[i + 1]].copy(),
                           "obs_index": r["idx"][o[i]:o[i + 1]].copy()} for i in range(nl)]}

    def recent_increase(self, kind, handles, d_found, d_visible):
        """IncreaseFound / IncreaseVisible of the named points (LMAP_POINT) or lines (LMAP_LINE) by the two deltas each"""
        hs = np.ascontiguousarray(handles, np.int32)
        df = np.ascontiguousarray(d_found, np.int32)
        dv = np.ascontiguousarray(d_visible, np.int32)
        assert hs.shape == df.shape == dv.shape
        self._chk(self.L.drfe_lmap_recent_increase(self.h, int(kind), len(hs), _p(hs), _p(df), _p(dv)), "drfe_lmap_recent_increase")

    def recent_cull(self, current_kf_id, points=(), lines=(), monocular=False, mode="batch", capacity=None):
        """MapPointCulling over `points` and MapLineCulling over `lines` (mlpRecentAddedMapPoints / mlpRecentAddedMapLines as
        handles, in list order) for mpCurrentKeyFrame->mnId = current_kf_id.  Returns a dict with "points" and "lines", each a
        dict: action [n], kept (the surviving list), culled (handles in list order), erased (per culled item an [m, 2] array of
        (key frame, index) in stored order).  capacity: (point observations, line observations) that may be erased; default:
        grown until the call fits (a call that does not fit changes nothing)."""
        fn = getattr(self.L, f"drfe_lmap_recent_cull_{mode}")
        hs = [np.ascontiguousarray(points, np.int32), np.ascontiguousarray(lines, np.int32)]
        grow = capacity is None
        caps = [1 << 12, 1 << 12] if grow else [int(c) for c in capacity]
        while True:
            arrs, lists = [], []
            for k in range(2):
                n = len(hs[k])
                a = {"action": np.zeros(max(1, n), np.uint8), "n_kept": np.zeros(1, np.int32), "kept": np.zeros(max(1, n), np.int32),
                     "n_culled": np.zeros(1, np.int32), "culled": np.zeros(max(1, n), np.int32),
                     "erased_offsets": np.zeros(n + 1, np.int32), "erased_kf": np.zeros(max(1, caps[k]), np.int32),
                     "erased_index": np.zeros(max(1, caps[k]), np.int32)}
                arrs.append(a)
                lists.append(LmapRecentList(n, _p(hs[k]), caps[k], *[_p(a[f]) for f in (
                    "action", "n_kept", "kept", "n_culled", "culled", "erased_offsets", "erased_kf", "erased_index")]))
            args = (self.h, int(current_kf_id), 1 if monocular else 0, C.byref(lists[0]), C.byref(lists[1])) + (
                () if mode == "host" else (None,))
            rc = fn(*args)
            if not (grow and rc == ERR_CAPACITY and caps[0] < (1 << 28)
                    and b"than erased_capacity" in self.L.drfe_lmap_last_error(self.h)):
                break
            caps = [v * 8 for v in caps]
        self._chk(rc, f"drfe_lmap_recent_cull_{mode}")
        res = {}
        for k, name in enumerate(("points", "lines")):
            a, n = arrs[k], len(hs[k])
            nk, nc, o = int(a["n_kept"][0]), int(a["n_culled"][0]), a["erased_offsets"]
            res[name] = dict(action=a["action"][:n].copy(), kept=a["kept"][:nk].copy(), culled=a["culled"][:nc].copy(),
                             erased=[np.stack([a["erased_kf"][o[i]:o[i + 1]], a["erased_index"][o[i]:o[i + 1]]], axis=1)
                                     for i in range(nc)])
        return res

    # ---- the fuse commit on the store ----

    @staticmethod
    def fuse_limits():
        out = np.zeros(8, np.int32)
        rc = load().drfe_lmap_fuse_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_fuse_limits failed ({rc})")
        return dict(zip(LMAP_FUSE_LIMITS, (int(v) for v in out)))

    def fuse_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_fuse_stats(self.h, _p(st)), "drfe_lmap_fuse_stats")
        return dict(zip(LMAP_FUSE_STATS, (int(v) for v in st)))

    def fuse_scratch(self, n_candidates, n_steps):
        """bytes of device scratch a fuse call takes at most: (the call, the same, the part every call takes)"""
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_fuse_scratch(self.h, int(n_candidates), int(n_steps), _p(out)), "drfe_lmap_fuse_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def get_replaced(self, kind, handles):
        hs = np.ascontiguousarray(handles, np.int32)
        out = np.zeros(max(1, len(hs)), np.int32)
        self._chk(self.L.drfe_lmap_get_replaced(self.h, int(kind), len(hs), _p(hs), _p(out)), "drfe_lmap_get_replaced")
        return out[:len(hs)].copy()

    def get_match_row(self, kind, keyframe):
        n = np.zeros(1, np.int32)
        rc = self.L.drfe_lmap_get_match_row(self.h, int(kind), int(keyframe), 0, _p(n), None)
        if rc not in (0, ERR_CAPACITY):
            self._chk(rc, "drfe_lmap_get_match_row")
        out = np.zeros(max(1, int(n[0])), np.int32)
        self._chk(self.L.drfe_lmap_get_match_row(self.h, int(kind), int(keyframe), len(out), _p(n), _p(out)), "drfe_lmap_get_match_row")
        return out[:int(n[0])].copy()

    def get_observers(self, kind, handle):
        """(bad, the observing key frames in stored order) of a map point or map line"""
        n, bad = np.zeros(1, np.int32), np.zeros(1, np.uint8)
        rc = self.L.drfe_lmap_get_observers(self.h, int(kind), int(handle), 0, _p(bad), _p(n), None)
        if rc not in (0, ERR_CAPACITY):
            self._chk(rc, "drfe_lmap_get_observers")
        out = np.zeros(max(1, int(n[0])), np.int32)
        self._chk(self.L.drfe_lmap_get_observers(self.h, int(kind), int(handle), len(out), _p(bad), _p(n), _p(out)),
                  "drfe_lmap_get_observers")
        return int(bad[0]), out[:int(n[0])].copy()

    def fuse(self, steps, mode="batch", capacity=None):
        """The fuse commit: steps are dicts with keyframe, kind (LMAP_POINT / LMAP_LINE), form (FUSE_NEIGHBOURS / FUSE_LOOP /
        FUSE_MATCHED), candidates (handles, -1 = null) and best_idx (not for FUSE_MATCHED).  Returns a dict: steps (per step a dict
        of action [n], n_fused and replace [n]), replaced (a list of (kind, loser, winner, records [m, 3] of (key frame, index,
        moved) in stored order)), touched_points, touched_lines.  capacity: (replacements, records, touched per kind); default:
        the documented bounds for the first and third and records grown until the call fits (a call that does not fit changes
        nothing)."""
        n = len(steps)
        S = (LmapFuseStep * max(1, n))()
        keep = []
        live = 0
        for i, st in enumerate(steps):
            cand = np.ascontiguousarray(st["candidates"], np.int32)
            m = len(cand)
            best = None if st["form"] == FUSE_MATCHED and "best_idx" not in st else np.ascontiguousarray(st["best_idx"], np.int32)
            a = {"cand": cand, "best": best, "action": np.zeros(max(1, m), np.uint8), "n_fused": np.zeros(1, np.int32),
                 "replace": np.full(max(1, m), -1, np.int32)}
            keep.append(a)
            live += int(np.count_nonzero(cand >= 0))
            S[i] = LmapFuseStep(int(st["keyframe"]), int(st["kind"]), int(st["form"]), m, _p(cand), None if best is None else _p(best),
                                _p(a["action"]), _p(a["n_fused"]), _p(a["replace"]))
        grow = capacity is None
        cr, crec, ct = (live, 1 << 12, live) if grow else (int(c) for c in capacity)
        fn = getattr(self.L, f"drfe_lmap_fuse_{mode}")
        while True:
            r = {"n_replaced": np.zeros(1, np.int32), "replaced_kind": np.zeros(max(1, cr), np.int32),
                 "loser": np.zeros(max(1, cr), np.int32), "winner": np.zeros(max(1, cr), np.int32),
                 "record_offsets": np.zeros(cr + 1, np.int32), "record_kf": np.zeros(max(1, crec), np.int32),
                 "record_index": np.zeros(max(1, crec), np.int32), "record_moved": np.zeros(max(1, crec), np.uint8),
                 "n_touched": np.zeros(2, np.int32), "touched_points": np.zeros(max(1, ct), np.int32),
                 "touched_lines": np.zeros(max(1, ct), np.int32)}
            call = LmapFuseCall(n, C.cast(S, C.c_void_p), cr, crec, ct, *[_p(r[k]) for k in (
                "n_replaced", "replaced_kind", "loser", "winner", "record_offsets", "record_kf", "record_index", "record_moved",
                "n_touched", "touched_points", "touched_lines")])
            args = (self.h, C.byref(call)) + (() if mode == "host" else (None,))
            rc = fn(*args)
            if not (grow and rc == ERR_CAPACITY and crec < (1 << 28) and b"record_capacity" in self.L.drfe_lmap_last_error(self.h)):
                break
            crec *= 8
        self._chk(rc, f"drfe_lmap_fuse_{mode}")
        nr, o = int(r["n_replaced"][0]), r["record_offsets"]
        return {"steps": [dict(action=a["action"][:len(a["cand"])].copy(), n_fused=int(a["n_fused"][0]),
                               replace=a["replace"][:len(a["cand"])].copy()) for a in keep],
                "replaced": [(int(r["replaced_kind"][i]), int(r["loser"][i]), int(r["winner"][i]),
                              np.stack([r["record_kf"][o[i]:o[i + 1]], r["record_index"][o[i]:o[i + 1]],
                                        r["record_moved"][o[i]:o[i + 1]].astype(np.int32)], axis=1)) for i in range(nr)],
                "touched_points": r["touched_points"][:int(r["n_touched"][0])].copy(),
                "touched_lines": r["touched_lines"][:int(r["n_touched"][1])].copy()}

    # ---- the item loops of LocalMapping::ProcessNewKeyFrame on the store ----

    @staticmethod
    def insert_limits():
        out = np.zeros(8, np.int32)
        rc = load().drfe_lmap_insert_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_insert_limits failed ({rc})")
        return dict(zip(LMAP_INSERT_LIMITS, (int(v) for v in out)))

    def insert_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_insert_stats(self.h, _p(st)), "drfe_lmap_insert_stats")
        return dict(zip(LMAP_INSERT_STATS, (int(v) for v in st)))

    def insert_scratch(self, handles, normals=True):
        """bytes of device scratch an insert call of these key frames takes: (as one chunk, with one key frame a chunk, the part
        every chunk shares)"""
        hs = np.ascontiguousarray(handles, np.int32)
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_insert_scratch(self.h, len(hs), _p(hs), int(bool(normals)), _p(out)), "drfe_lmap_insert_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def insert(self, handles, mode="batch", normals=True, capacity=None):
        """The item loops of ProcessNewKeyFrame for the key frames `handles` in queue order.  Returns a dict: point_action and
        line_action (per called key frame an array of action bytes, INSERT_NULL / _BAD / _RECENT / _ADDED), added_points [m, 3] and
        added_lines [m, 3] of (item, key frame, index) in walk order, recent_points and recent_lines (handles in push order) and,
        with normals, normal [m, 3], max_distance, min_distance and status per added point.  capacity: (action, added, recent)
        entries per kind; default: grown until the call fits (a call that does not fit changes nothing)."""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        grow = capacity is None
        ca, cd, cr = (1 << 12, 1 << 12, 1 << 12) if grow else (int(c) for c in capacity)
        fn = getattr(self.L, f"drfe_lmap_insert_{mode}")
        while True:
            r = {"point_offsets": np.zeros(n + 1, np.int32), "point_action": np.zeros(max(1, ca), np.uint8),
                 "line_offsets": np.zeros(n + 1, np.int32), "line_action": np.zeros(max(1, ca), np.uint8),
                 "n_added": np.zeros(2, np.int32), "added_points": np.zeros(max(1, cd), np.int32),
                 "added_point_kf": np.zeros(max(1, cd), np.int32), "added_point_index": np.zeros(max(1, cd), np.int32),
                 "normal": np.zeros((max(1, cd), 3), np.float32) if normals else None, "max_distance": np.zeros(max(1, cd), np.float32),
                 "min_distance": np.zeros(max(1, cd), np.float32), "status": np.zeros(max(1, cd), np.uint8),
                 "added_lines": np.zeros(max(1, cd), np.int32), "added_line_kf": np.zeros(max(1, cd), np.int32),
                 "added_line_index": np.zeros(max(1, cd), np.int32), "n_recent": np.zeros(2, np.int32),
                 "recent_points": np.zeros(max(1, cr), np.int32), "recent_lines": np.zeros(max(1, cr), np.int32)}
            call = LmapInsertCall(n, 0, _p(hs), (C.c_int32 * 2)(ca, ca), (C.c_int32 * 2)(cd, cd), (C.c_int32 * 2)(cr, cr),
                                  *[None if r[k] is None else _p(r[k]) for k in LMAP_INSERT_CALL_FIELDS])
            args = (self.h, C.byref(call)) + (() if mode == "host" else (None,))
            rc = fn(*args)
            if not (grow and rc == ERR_CAPACITY and ca < (1 << 28) and b"_capacity[" in self.L.drfe_lmap_last_error(self.h)):
                break
            ca, cd, cr = ca * 8, cd * 8, cr * 8
        self._chk(rc, f"drfe_lmap_insert_{mode}")
        po, lo = r["point_offsets"], r["line_offsets"]
        ap, al = int(r["n_added"][0]), int(r["n_added"][1])
        res = {"point_action": [r["point_action"][po[j]:po[j + 1]].copy() for j in range(n)],
               "line_action": [r["line_action"][lo[j]:lo[j + 1]].copy() for j in range(n)],
               "added_points": np.stack([r["added_points"][:ap], r["added_point_kf"][:ap], r["added_point_index"][:ap]], axis=1),
               "added_lines": np.stack([r["added_lines"][:al], r["added_line_kf"][:al], r["added_line_index"][:al]], axis=1),
               "recent_points": r["recent_points"][:int(r["n_recent"][0])].copy(),
               "recent_lines": r["recent_lines"][:int(r["n_recent"][1])].copy()}
        if normals:
            res.update({k: r[k][:ap].copy() for k in ("normal", "max_distance", "min_distance", "status")})
        return res

    # ---- map-point and map-line creation on the store, appended in place ----

    @staticmethod
    def create_limits():
        out = np.zeros(8, np.int32)
        rc = load().drfe_lmap_create_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_create_limits failed ({rc})")
        return dict(zip(LMAP_CREATE_LIMITS, (int(v) for v in out)))

    def create_scratch(self, n_points, n_lines=0):
        """bytes of device scratch a create call of that many creations takes: (each kind as one chunk, with one workgroup of
        creations a chunk, the part every chunk shares)"""
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_create_scratch(self.h, int(n_points), int(n_lines), _p(out)), "drfe_lmap_create_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def create_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_create_stats(self.h, _p(st)), "drfe_lmap_create_stats")
        return dict(zip(LMAP_CREATE_STATS, (int(v) for v in st)))

    def create(self, points=(), lines=(), mode="batch", normals=True, capacity=None):
        """The tail of CreateNewMapPoints / CreateNewMapLines2 for the creations `points`, then `lines`, in order.  A creation is
        a dict: handle, obs (1 or 2 (key frame, index) pairs in the caller's order), ref_kf, first_kf and, for a point, world.
        Returns a dict: point_displaced and line_displaced [n, 2] (the handle that stood in the row entry of each observation, -1
        for none) and, with normals, normal [n, 3], max_distance, min_distance and status per created point.  capacity:
        (displaced entries per kind, records); default: what the call needs."""
        fn = getattr(self.L, f"drfe_lmap_create_{mode}")
        def pack(items, point):
            n = len(items)
            r = {"handle": np.zeros(n, np.int32), "n_obs": np.zeros(n, np.int32), "obs_kf": np.zeros((n, 2), np.int32),
                 "obs_index": np.zeros((n, 2), np.int32), "ref_kf": np.zeros(n, np.int32), "first_kf": np.zeros(n, np.int64)}
            if point:
                r["world"] = np.zeros((n, 3), np.float32)
            for t, it in enumerate(items):
                r["handle"][t], r["ref_kf"][t], r["first_kf"][t] = it["handle"], it["ref_kf"], it.get("first_kf", 0)
                obs = list(it["obs"])
                r["n_obs"][t] = len(obs)
                for o, (k, i) in enumerate(obs[:2]):
                    r["obs_kf"][t, o], r["obs_index"][t, o] = k, i
                if point:
                    r["world"][t] = it["world"]
            return r
        points, lines = list(points), list(lines)
        a = {"point_" + k: v for k, v in pack(points, True).items()}
        a.update({"line_" + k: v for k, v in pack(lines, False).items()})
        nP, nL = len(points), len(lines)
        cd, cr = (2 * max(nP, nL), nP) if capacity is None else (int(v) for v in capacity)
        out = {"point_displaced": np.full((max(1, nP), 2), -1, np.int32), "line_displaced": np.full((max(1, nL), 2), -1, np.int32),
               "normal": np.zeros((max(1, nP), 3), np.float32) if normals else None, "max_distance": np.zeros(max(1, nP), np.float32),
               "min_distance": np.zeros(max(1, nP), np.float32), "status": np.zeros(max(1, nP), np.uint8)}
        call = LmapCreateCall(nP, nL, *[_p(a[k]) for k in LMAP_CREATE_IN_FIELDS], (C.c_int32 * 2)(cd, cd), cr, 0,
                              *[None if out[k] is None else _p(out[k]) for k in LMAP_CREATE_OUT_FIELDS])
        self._chk(fn(*((self.h, C.byref(call)) + (() if mode == "host" else (None,)))), f"drfe_lmap_create_{mode}")
        res = {"point_displaced": out["point_displaced"][:nP].copy(), "line_displaced": out["line_displaced"][:nL].copy()}
        if normals:
            res.update({k: out[k][:nP].copy() for k in ("normal", "max_distance", "min_distance", "status")})
        return res

    # ---- what surrounds the solver of Optimizer::OptimizeEssentialGraph on the store ----

    @staticmethod
    def essential_limits():
        out = np.zeros(8, np.int32)
        rc = load().drfe_lmap_essential_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_essential_limits failed ({rc})")
        return dict(zip(LMAP_ESSENTIAL_LIMITS, (int(v) for v in out)))

    def essential_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_essential_stats(self.h, _p(st)), "drfe_lmap_essential_stats")
        return dict(zip(LMAP_ESSENTIAL_STATS, (int(v) for v in st)))

    def essential_scratch(self, lc_entries=0):
        """bytes of device scratch on the store as it is: dict of edges (an edges call with that many loop-connection members, as a
        whole), edges_fixed, commit_whole, commit_least, commit_fixed, and edge_bound (the edges the bound counts)"""
        out = np.zeros(6, np.int64)
        self._chk(self.L.drfe_lmap_essential_scratch(self.h, int(lc_entries), _p(out)), "drfe_lmap_essential_scratch")
        return dict(zip(("edges", "edges_fixed", "commit_whole", "commit_least", "commit_fixed", "edge_bound"), (int(v) for v in out)))

    def essential_upload_bytes(self):
        """host-to-device bytes of the loop-edge block since the store was made"""
        out = np.zeros(1, np.int64)
        self._chk(self.L.drfe_lmap_essential_upload_bytes(self.h, _p(out)), "drfe_lmap_essential_upload_bytes")
        return int(out[0])

    def set_loop_edges(self, rows):
        """rows: (handle, [loop-edge handles]) pairs: mspLoopEdges of each key frame; a row replaces the stored one"""
        rows = [(int(h), [int(e) for e in es]) for h, es in rows]
        hs = np.array([h for h, _ in rows], np.int32)
        off = np.zeros(len(rows) + 1, np.int32)
        off[1:] = np.cumsum([len(es) for _, es in rows])
        ed = np.array([e for _, es in rows for e in es], np.int32)
        self._chk(self.L.drfe_lmap_set_loop_edges(self.h, len(hs), _p(hs), _p(off), _p(ed) if len(ed) else None),
                  "drfe_lmap_set_loop_edges")

    def get_loop_edges(self, handles):
        """the stored rows, each in ascending rank: a list of int32 arrays"""
        hs = np.ascontiguousarray(handles, np.int32)
        off = np.zeros(len(hs) + 1, np.int32)
        ed = np.zeros(64, np.int32)
        rc = self.L.drfe_lmap_get_loop_edges(self.h, len(hs), _p(hs), len(ed), _p(off), _p(ed))
        if rc == ERR_CAPACITY:
            ed = np.zeros(int(off[len(hs)]), np.int32)
            rc = self.L.drfe_lmap_get_loop_edges(self.h, len(hs), _p(hs), len(ed), _p(off), _p(ed))
        self._chk(rc, "drfe_lmap_get_loop_edges")
        return [ed[off[i]:off[i + 1]].copy() for i in range(len(hs))]

    def essential_edges(self, loop_kf, cur_kf, sim3=(), loop_connections=(), mode="batch", capacity=None):
        """The vertices and the ordered edge list of OptimizeEssentialGraph (src/Optimizer.cc:2910-3080).  sim3: (handle, corrected,
        non_corrected) rows, each Sim3 as (qx, qy, qz, qw, tx, ty, tz, s); loop_connections: (key, [members]) rows.  Returns a dict:
        per vertex in rank order vertices, Scw [v, 8], fixed; per edge in addEdge order from, to, measurement [e, 8], kind.
        capacity: (vertices, edges), default the bound that always suffices.  The store is not changed."""
        sim3, lcs = list(sim3), [(int(k), [int(m) for m in ms]) for k, ms in loop_connections]
        a = {"sim3_handles": np.array([r[0] for r in sim3], np.int32),
             "corrected": np.array([r[1] for r in sim3], np.float64).reshape(len(sim3), 8),
             "non_corrected": np.array([r[2] for r in sim3], np.float64).reshape(len(sim3), 8),
             "lc_handles": np.array([k for k, _ in lcs], np.int32), "lc_offsets": np.zeros(len(lcs) + 1, np.int32),
             "lc_kfs": np.array([m for _, ms in lcs for m in ms], np.int32)}
        a["lc_offsets"][1:] = np.cumsum([len(ms) for _, ms in lcs])
        if capacity is None:
            capacity = (self.size()[0], self.essential_scratch(len(a["lc_kfs"]))["edge_bound"])
        cv, ce = (int(v) for v in capacity)
        v, e = max(1, cv), max(1, ce)
        r = {"n_vertices": np.zeros(1, np.int32), "vertices": np.zeros(v, np.int32), "Scw": np.zeros((v, 8), np.float64),
             "fixed": np.zeros(v, np.uint8), "n_edges": np.zeros(1, np.int32), "from": np.zeros(e, np.int32), "to": np.zeros(e, np.int32),
             "measurement": np.zeros((e, 8), np.float64), "kind": np.zeros(e, np.uint8)}
        call = LmapEssentialEdgesCall(int(loop_kf), int(cur_kf), len(sim3), len(lcs),
                                      *[_p(a[k]) if len(a[k]) else None for k in LMAP_ESSENTIAL_EDGES_IN[:3]],
                                      *[_p(a[k]) for k in LMAP_ESSENTIAL_EDGES_IN[3:]], cv, ce,
                                      *[_p(r[k]) for k in LMAP_ESSENTIAL_EDGES_OUT])
        fn = getattr(self.L, f"drfe_lmap_essential_edges_{mode}")
        self._chk(fn(*((self.h, C.byref(call)) + (() if mode == "host" else (None,)))), f"drfe_lmap_essential_edges_{mode}")
        nv, ne = int(r["n_vertices"][0]), int(r["n_edges"][0])
        res = {k: r[k][:nv].copy() for k in ("vertices", "Scw", "fixed")}
        res.update({k: r[k][:ne].copy() for k in ("from", "to", "measurement", "kind")})
        return res

    def essential_commit(self, cur_kf, handles, Scw, optimised, mode="batch", capacity=None):
        """The tail of OptimizeEssentialGraph (src/Optimizer.cc:3088-3131): the vertices `handles` with the Scw the edges call gave
        and the solver's estimates `optimised` [n, 8].  Returns a dict: per named key frame Tiw [n, 4, 4] and Swc [n, 8]
        (vCorrectedSwc, for the caller's lines and planes); per moved point in ascending handle points, ref (nIDr), world, normal,
        max_distance, min_distance, status.  capacity: moved points, default the stored points.  Commits poses and positions."""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        S = np.ascontiguousarray(Scw, np.float64).reshape(n, 8)
        O = np.ascontiguousarray(optimised, np.float64).reshape(n, 8)
        cap = self.size()[1] if capacity is None else int(capacity)
        k, m = max(1, n), max(1, cap)
        r = {"Tiw": np.zeros((k, 4, 4), np.float32), "Swc": np.zeros((k, 8), np.float64), "n_points": np.zeros(1, np.int32),
             "points": np.zeros(m, np.int32), "ref": np.zeros(m, np.int32), "world": np.zeros((m, 3), np.float32),
             "normal": np.zeros((m, 3), np.float32), "max_distance": np.zeros(m, np.float32), "min_distance": np.zeros(m, np.float32),
             "status": np.zeros(m, np.uint8)}
        call = LmapEssentialCommitCall(int(cur_kf), n, _p(hs), _p(S), _p(O), cap, 0, *[_p(r[f]) for f in LMAP_ESSENTIAL_COMMIT_OUT])
        fn = getattr(self.L, f"drfe_lmap_essential_commit_{mode}")
        self._chk(fn(*((self.h, C.byref(call)) + (() if mode == "host" else (None,)))), f"drfe_lmap_essential_commit_{mode}")
        nm = int(r["n_points"][0])
        res = {f: r[f][:n].copy() for f in ("Tiw", "Swc")}
        res.update({f: r[f][:nm].copy() for f in LMAP_ESSENTIAL_COMMIT_OUT[3:]})
        return res

    # ---- the map update of LoopClosing::RunGlobalBundleAdjustment on the store ----

    @staticmethod
    def gba_limits():
        out = np.zeros(6, np.int32)
        rc = load().drfe_lmap_gba_limits(_p(out))
        if rc != 0:
            raise DrfeError(f"drfe_lmap_gba_limits failed ({rc})")
        return dict(zip(LMAP_GBA_LIMITS, (int(v) for v in out)))

    def gba_stats(self):
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_lmap_gba_stats(self.h, _p(st)), "drfe_lmap_gba_stats")
        return dict(zip(LMAP_GBA_STATS, (int(v) for v in st)))

    def gba_scratch(self):
        """bytes of device scratch a gba call takes: (as one chunk, at least, shared by every chunk)"""
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_gba_scratch(self.h, _p(out)), "drfe_lmap_gba_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def set_gba_keyframes(self, handles, TcwGBA, stamps):
        """mTcwGBA [n, 4, 4] float32 and mnBAGlobalForKF (handles) as the adjustment's write-back left them"""
        hs = np.ascontiguousarray(handles, np.int32)
        T = np.ascontiguousarray(TcwGBA, np.float32).reshape(len(hs), 16)
        st = np.ascontiguousarray(stamps, np.int32).reshape(len(hs))
        self._chk(self.L.drfe_lmap_set_gba_keyframes(self.h, len(hs), _p(hs), _p(T), _p(st)), "drfe_lmap_set_gba_keyframes")

    def set_gba_points(self, handles, PosGBA, stamps):
        """mPosGBA [n, 3] float32 and mnBAGlobalForKF (handles)"""
        hs = np.ascontiguousarray(handles, np.int32)
        X = np.ascontiguousarray(PosGBA, np.float32).reshape(len(hs), 3)
        st = np.ascontiguousarray(stamps, np.int32).reshape(len(hs))
        self._chk(self.L.drfe_lmap_set_gba_points(self.h, len(hs), _p(hs), _p(X), _p(st)), "drfe_lmap_set_gba_points")

    def get_gba_keyframes(self, handles):
        """dict of TcwGBA [n, 4, 4], stamp [n], TcwBefGBA [n, 4, 4], has_TcwGBA [n], has_TcwBefGBA [n]"""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        r = {"TcwGBA": np.zeros((n, 4, 4), np.float32), "stamp": np.zeros(n, np.int32), "TcwBefGBA": np.zeros((n, 4, 4), np.float32),
             "has_TcwGBA": np.zeros(n, np.uint8), "has_TcwBefGBA": np.zeros(n, np.uint8)}
        self._chk(self.L.drfe_lmap_get_gba_keyframes(self.h, n, _p(hs), *[_p(v) for v in r.values()]), "drfe_lmap_get_gba_keyframes")
        return r

    def get_gba_points(self, handles):
        """dict of PosGBA [n, 3], stamp [n], has_PosGBA [n]"""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        r = {"PosGBA": np.zeros((n, 3), np.float32), "stamp": np.zeros(n, np.int32), "has_PosGBA": np.zeros(n, np.uint8)}
        self._chk(self.L.drfe_lmap_get_gba_points(self.h, n, _p(hs), *[_p(v) for v in r.values()]), "drfe_lmap_get_gba_points")
        return r

    def gba(self, loop, origins, mode="batch", capacity=None):
        """The map update after a global bundle adjustment (src/LoopClosing.cc:722-783) for nLoopKF = `loop` from the origin key
        frames.  Returns a dict: per visited key frame in the reference's FIFO order keyframes, Tcw [v, 4, 4], TcwBef [v, 4, 4],
        composed; per moved point in ascending handle points, world [m, 3], kind.  capacity: (key frames, points), default the
        sizes of the store (a call that does not fit changes nothing)."""
        og = np.ascontiguousarray(origins, np.int32)
        if capacity is None:
            nk, npt, _ = self.size()
            capacity = (nk, npt)
        ck, cp = (int(c) for c in capacity)
        k, m = max(1, ck), max(1, cp)
        r = {"n_keyframes": np.zeros(1, np.int32), "keyframes": np.zeros(k, np.int32), "Tcw": np.zeros((k, 4, 4), np.float32),
             "TcwBef": np.zeros((k, 4, 4), np.float32), "composed": np.zeros(k, np.uint8), "n_points": np.zeros(1, np.int32),
             "points": np.zeros(m, np.int32), "world": np.zeros((m, 3), np.float32), "kind": np.zeros(m, np.uint8)}
        out = LmapGbaOut(ck, cp, *[_p(r[f]) for f in LMAP_GBA_OUT_FIELDS])
        fn = getattr(self.L, f"drfe_lmap_gba_{mode}")
        args = (self.h, int(loop), len(og), _p(og), C.byref(out)) + (() if mode == "host" else (None,))
        self._chk(fn(*args), f"drfe_lmap_gba_{mode}")
        nv, nm = int(r["n_keyframes"][0]), int(r["n_points"][0])
        res = {f: r[f][:nv].copy() for f in ("keyframes", "Tcw", "TcwBef", "composed")}
        res.update({f: r[f][:nm].copy() for f in ("points", "world", "kind")})
        return res

    def cull_scratch(self, handles):
        """bytes of device scratch a cull call of these key frames takes: (as one chunk, at least, shared by every chunk)"""
        hs = np.ascontiguousarray(handles, np.int32)
        out = np.zeros(3, np.int64)
        self._chk(self.L.drfe_lmap_cull_scratch(self.h, len(hs), _p(hs), _p(out)), "drfe_lmap_cull_scratch")
        return int(out[0]), int(out[1]), int(out[2])

    def set_cull_attributes(self, kfs=(), points=()):
        """kfs: dicts with handle, th_depth, and optionally flags (CULL_NOT_ERASE | CULL_ORIGIN | CULL_TO_BE_ERASED) and octave,
        depth, stereo parallel to the match row.  points: dicts with handle, n_obs and obs_index parallel to the observations."""
        kh = np.array([r["handle"] for r in kfs], np.int32)
        th = np.array([r["th_depth"] for r in kfs], np.float32)
        fl = np.array([r.get("flags", 0) for r in kfs], np.uint8)
        roff, octv = _csr_i32([r.get("octave", ()) for r in kfs])
        dep = np.ascontiguousarray(np.concatenate([np.asarray(r.get("depth", ()), np.float32).reshape(-1) for r in kfs])
                                   if len(kfs) else [], np.float32)
        ste = np.ascontiguousarray(np.concatenate([np.asarray(r.get("stereo", ()), np.uint8).reshape(-1) for r in kfs])
                                   if len(kfs) else [], np.uint8)
        if len(dep) != len(octv) or len(ste) != len(octv):
            raise ValueError("octave, depth and stereo of a key frame must have one length")
        ph = np.array([r["handle"] for r in points], np.int32)
        nobs = np.array([r["n_obs"] for r in points], np.int32)
        ooff, oidx = _csr_i32([r.get("obs_index", ()) for r in points])
        A = LmapCullAttributes(len(kh), len(ph), _p(kh), _p(th), _p(fl), _p(roff), _p(octv), _p(dep), _p(ste), _p(ph), _p(nobs),
                               _p(ooff), _p(oidx))
        self._chk(self.L.drfe_lmap_set_cull_attributes(self.h, C.byref(A)), "drfe_lmap_set_cull_attributes")

    def get_cull_attributes(self, kf_handles=(), point_handles=()):
        """the stored attributes: dict of kfs (dicts with handle, th_depth, flags, octave, depth, stereo) and points (dicts with
        handle, n_obs, obs_index)"""
        kh = np.ascontiguousarray(kf_handles, np.int32)
        ph = np.ascontiguousarray(point_handles, np.int32)
        nk, npt = len(kh), len(ph)
        cap = 1 << 12
        while True:
            r = {"th_depth": np.zeros(max(1, nk), np.float32), "kf_flags": np.zeros(max(1, nk), np.uint8),
                 "row_offsets": np.zeros(nk + 1, np.int32), "octave": np.zeros(cap, np.int32), "depth": np.zeros(cap, np.float32),
                 "stereo": np.zeros(cap, np.uint8), "n_obs": np.zeros(max(1, npt), np.int32),
                 "obs_offsets": np.zeros(npt + 1, np.int32), "obs_index": np.zeros(cap, np.int32)}
            O = LmapCullAttributesOut(nk, npt, cap, cap, _p(kh), _p(r["th_depth"]), _p(r["kf_flags"]), _p(r["row_offsets"]),
                                      _p(r["octave"]), _p(r["depth"]), _p(r["stereo"]), _p(ph), _p(r["n_obs"]), _p(r["obs_offsets"]),
                                      _p(r["obs_index"]))
            rc = self.L.drfe_lmap_get_cull_attributes(self.h, C.byref(O))
            if rc != ERR_CAPACITY or cap >= (1 << 28):
                break
            cap *= 8
        self._chk(rc, "drfe_lmap_get_cull_attributes")
        ro, oo = r["row_offsets"], r["obs_offsets"]
        return {"kfs": [{"handle": int(kh[i]), "th_depth": r["th_depth"][i], "flags": int(r["kf_flags"][i]),
                         "octave": r["octave"][ro[i]:ro[i + 1]].copy(), "depth": r["depth"][ro[i]:ro[i + 1]].copy(),
                         "stereo": r["stereo"][ro[i]:ro[i + 1]].copy()} for i in range(nk)],
                "points": [{"handle": int(ph[i]), "n_obs": int(r["n_obs"][i]), "obs_index": r["obs_index"][oo[i]:oo[i + 1]].copy()}
                           for i in range(npt)]}

    def cull(self, handles, monocular=False, mode="batch", capacity=None):
        """KeyFrameCulling over `handles` (GetVectorCovisibleKeyFrames() of the current key frame, in that order).  Returns a dict:
        per called key frame record [n, 4] (nMPs, nRedundant, verdict, action), Tcp [n, 4, 4], has_Tcp [n]; culled (handles in
        order); per touched key frame (ascending rank) touched, flags, parent, first, weights, ordered, children, nulled; per
        touched point (ascending handle) points, point_n_obs, point_ref, point_bad, obs and obs_index (one array per point).
        capacity: (touched, weights, ordered, children, nulled, points, obs); default: arrays grown until the call fits (a call
        that does not fit changes nothing)."""
        hs = np.ascontiguousarray(handles, np.int32)
        n = len(hs)
        fn = getattr(self.L, f"drfe_lmap_cull_{mode}")
        grow = capacity is None
        caps = [1 << 10, 1 << 14, 1 << 14, 1 << 12, 1 << 12, 1 << 12, 1 << 14] if grow else [int(c) for c in capacity]
        while True:
            ct, cw, co, cch, cnu, cp, cob = caps
            r, rows = self._conn_rows(ct, cw, co)
            c = {"record": np.zeros((max(1, n), 4), np.int32), "Tcp": np.zeros((max(1, n), 4, 4), np.float32),
                 "has_Tcp": np.zeros(max(1, n), np.uint8), "n_culled": np.zeros(1, np.int32), "culled": np.zeros(max(1, n), np.int32),
                 "n_touched": np.zeros(1, np.int32), "touched": np.zeros(max(1, ct), np.int32), "flags": np.zeros(max(1, ct), np.uint8),
                 "children_offsets": np.zeros(ct + 1, np.int32), "children": np.zeros(max(1, cch), np.int32),
                 "nulled_offsets": np.zeros(ct + 1, np.int32), "nulled": np.zeros(max(1, cnu), np.int32),
                 "n_points": np.zeros(1, np.int32), "points": np.zeros(max(1, cp), np.int32),
                 "point_n_obs": np.zeros(max(1, cp), np.int32), "point_ref": np.zeros(max(1, cp), np.int32),
                 "point_bad": np.zeros(max(1, cp), np.uint8), "obs_offsets": np.zeros(cp + 1, np.int32),
                 "obs": np.zeros(max(1, cob), np.int32), "obs_index": np.zeros(max(1, cob), np.int32)}
            out = LmapCullOut(ct, cch, cnu, cp, cob, 0, _p(c["record"]), _p(c["Tcp"]), _p(c["has_Tcp"]), _p(c["n_culled"]),
                              _p(c["culled"]), _p(c["n_touched"]), _p(c["touched"]), rows, _p(c["flags"]), _p(c["children_offsets"]),
                              _p(c["children"]), _p(c["nulled_offsets"]), _p(c["nulled"]), _p(c["n_points"]), _p(c["points"]),
                              _p(c["point_n_obs"]), _p(c["point_ref"]), _p(c["point_bad"]), _p(c["obs_offsets"]), _p(c["obs"]),
                              _p(c["obs_index"]))
            args = (self.h, n, _p(hs), 1 if monocular else 0, C.byref(out)) + (() if mode == "host" else (None,))
            rc = fn(*args)
            if not (grow and rc == ERR_CAPACITY and caps[0] < (1 << 26)
                    and b"the call returns more than" in self.L.drfe_lmap_last_error(self.h)):
                break
            caps = [v * 8 for v in caps]
        self._chk(rc, f"drfe_lmap_cull_{mode}")
        nt, npt, nc = int(c["n_touched"][0]), int(c["n_points"][0]), int(c["n_culled"][0])
        res = self._conn_unpack(r, nt)
        co_, no_, oo = c["children_offsets"], c["nulled_offsets"], c["obs_offsets"]
        res.update(record=c["record"][:n].copy(), Tcp=c["Tcp"][:n].copy(), has_Tcp=c["has_Tcp"][:n].copy(),
                   culled=c["culled"][:nc].copy(), touched=c["touched"][:nt].copy(), flags=c["flags"][:nt].copy(),
                   children=[c["children"][co_[k]:co_[k + 1]].copy() for k in range(nt)],
                   nulled=[c["nulled"][no_[k]:no_[k + 1]].copy() for k in range(nt)],
                   points=c["points"][:npt].copy(), point_n_obs=c["point_n_obs"][:npt].copy(),
                   point_ref=c["point_ref"][:npt].copy(), point_bad=c["point_bad"][:npt].copy(),
                   obs=[c["obs"][oo[k]:oo[k + 1]].copy() for k in range(npt)],
                   obs_index=[c["obs_index"][oo[k]:oo[k + 1]].copy() for k in range(npt)])
        return res


class Shard:
    """drfe_shard_*: the native (RCCL) side of the batched-sequence mode - what a C++ host calls where bench.py uses
    torch.distributed: unique id on rank 0, communicator per rank, broadcast of host buffers (the vocabulary), end-of-run
    MAX / SUM reduction."""

    @staticmethod
    def unique_id():
        L = load()
        ident = np.zeros(128, np.uint8)
        rc = L.drfe_shard_unique_id(_p(ident))
        if rc != 0:
            raise DrfeError(f"drfe_shard_unique_id failed ({rc}): {L.drfe_shard_last_error(None).decode()}")
        return ident

    @staticmethod
    def sequences_of_rank(n_sequences, nranks, rank):
        L = load()
        out = np.zeros(max(1, n_sequences), np.int32)
        n = L.drfe_shard_sequences_of_rank(n_sequences, nranks, rank, _p(out), len(out))
        if n < 0:
            raise DrfeError(f"drfe_shard_sequences_of_rank failed ({n})")
        return out[:n].copy()

    def __init__(self, ident, nranks, rank, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.drfe_shard_create(_p(np.ascontiguousarray(ident, np.uint8)), nranks, rank, device, C.byref(h))
        if rc != 0:
            raise DrfeError(f"drfe_shard_create failed ({rc}): {self.L.drfe_shard_last_error(None).decode()}")
        self.h = h

    def _chk(self, rc, what):
        if rc != 0:
            raise DrfeError(f"{what} failed ({rc}): {self.L.drfe_shard_last_error(self.h).decode()}")

    def broadcast(self, arr: np.ndarray, root=0):
        """in place: a C-contiguous host array from rank `root` to every rank"""
        assert arr.flags.c_contiguous
        self._chk(self.L.drfe_shard_broadcast(self.h, _p(arr), arr.nbytes, root), "drfe_shard_broadcast")
        return arr

    def reduce_report(self, maxima, sums):
        m = np.ascontiguousarray(maxima, np.float64).copy()
        s = np.ascontiguousarray(sums, np.int64).copy()
        self._chk(self.L.drfe_shard_reduce_report(self.h, _p(m), len(m), _p(s), len(s)), "drfe_shard_reduce_report")
        return m, s

    def close(self):
        if getattr(self, "h", None):
            self.L.drfe_shard_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """drfe_pipeline: `depth` contexts used round robin, each on its own stream (batches in flight)."""

    def __init__(self, depth, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th_fast=20, min_th_fast=7, max_width=640, max_height=480,
                 max_batch=1, device=0):
        self.L = load()
        self.cfg = Config(device, max_width, max_height, max_batch, nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast)
        h = C.c_void_p()
        rc = self.L.drfe_pipeline_create(C.byref(self.cfg), depth, C.byref(h))
        if rc != 0:
            raise DrfeError(f"drfe_pipeline_create failed ({rc}): {self.L.drfe_last_error(None).decode()}")
        self.h = h
        self.depth = self.L.drfe_pipeline_depth(self.h)
        self.contexts = [Context.view(self.L.drfe_pipeline_context(self.h, k), nlevels, max_batch) for k in range(self.depth)]

    def submit(self, d_gray: int, d_depth: int, frame_stride: int, row_stride: int, w: int, h: int, Tcw, Twc, cam, th=15.0, mono=False,
               check_ori=True, nframes=1) -> int:
        """-> index of the context that holds this batch's results"""
        t1 = np.ascontiguousarray(Tcw, np.float32) if Tcw is not None else None
        t2 = np.ascontiguousarray(Twc, np.float32) if Twc is not None else None
        k = self.L.drfe_pipeline_submit(self.h, C.c_void_p(d_gray), C.c_void_p(d_depth) if d_depth else None, frame_stride, row_stride, w, h,
                                        _p(t1) if t1 is not None else None, _p(t2) if t2 is not None else None,
                                        C.byref(cam) if cam is not None else None, th, int(mono), int(check_ori), nframes)
        if k < 0:
            raise DrfeError(f"drfe_pipeline_submit failed ({k}): {self.L.drfe_pipeline_last_error(self.h).decode()}")
        return k

    def sync(self, k=-1):
        rc = self.L.drfe_pipeline_sync(self.h, k)
        if rc != 0:
            raise DrfeError(f"drfe_pipeline_sync failed ({rc}): {self.L.drfe_pipeline_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            for c in self.contexts:
                c.close()
            self.L.drfe_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns one drfe_ctx (one HIP device, one batch arena)."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th_fast=20, min_th_fast=7,
                 max_width=640, max_height=480, max_batch=1, device=0):
        self.L = load()
        self.cfg = Config(device, max_width, max_height, max_batch, nfeatures, scale_factor, nlevels, ini_th_fast,
                          min_th_fast)
        h = C.c_void_p()
        rc = self.L.drfe_create(C.byref(self.cfg), C.byref(h))
        if rc != 0:
            raise DrfeError(f"drfe_create failed ({rc}): {self.L.drfe_last_error(None).decode()}")
        self.h = h
        self.nlevels = nlevels
        self.max_kp = self.L.drfe_orb_max_keypoints(self.h)
        self.max_batch = max_batch

    @classmethod
    def view(cls, handle, nlevels, max_batch):
        """A Context over a drfe_ctx somebody else owns (a pipeline's): same methods, close() does not destroy it."""
        self = cls.__new__(cls)
        self.L = load()
        self.h = C.c_void_p(handle)
        self.owned = False
        self.nlevels = nlevels
        self.max_kp = self.L.drfe_orb_max_keypoints(self.h)
        self.max_batch = max_batch
        return self

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "owned", True):
                self.L.drfe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise DrfeError(f"{what} failed ({rc}): {self.L.drfe_last_error(self.h).decode()}")

    # --- ORB ---------------------------------------------------------------------------------------
    def scale_tables(self):
        t = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        self._chk(self.L.drfe_orb_scale_tables(self.h, *[_p(a) for a in t]), "drfe_orb_scale_tables")
        return t

    def orb_extract(self, gray: np.ndarray):
        """Single host frame -> (keypoints structured array, descriptors [N,32] uint8)."""
        if gray is None or gray.size == 0:
            n = C.c_int(0)
            self._chk(self.L.drfe_orb_extract(self.h, None, 0, 0, 0, None, None, 0, C.byref(n)), "drfe_orb_extract")
            return np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.strides[1] == 1
        kps = np.zeros(self.max_kp, KP_DTYPE)
        desc = np.zeros((self.max_kp, 32), np.uint8)
        n = C.c_int(0)
        self._chk(self.L.drfe_orb_extract(self.h, _p(gray), gray.shape[1], gray.shape[0], gray.strides[0], _p(kps),
                                          _p(desc), self.max_kp, C.byref(n)), "drfe_orb_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def frame_submit(self, slot: int, gray: np.ndarray, depth16: np.ndarray = None, cam: Camera = None):
        """Per-frame pipelined flow: enqueue ORB (+ the Frame glue when a raw depth image is given) of one host frame into
        `slot` and return without waiting."""
        assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.strides[1] == 1
        dp, ds = None, 0
        if depth16 is not None:
            assert depth16.dtype == np.uint16 and depth16.shape == gray.shape and depth16.strides[1] == 2
            dp, ds = _p(depth16), depth16.strides[0] // 2
        self._chk(self.L.drfe_frame_submit(self.h, slot, _p(gray), gray.shape[1], gray.shape[0], gray.strides[0], dp,
                                           C.c_size_t(ds), C.byref(cam) if cam is not None else None), "drfe_frame_submit")

    def frame_collect(self, slot: int, stereo=False):
        """-> (mvKeys, mDescriptors[, mvuRight, mvDepth]) of the slot's outstanding submission."""
        kps = np.zeros(self.max_kp, KP_DTYPE)
        desc = np.zeros((self.max_kp, 32), np.uint8)
        ur = np.zeros(self.max_kp, np.float32) if stereo else None
        z = np.zeros(self.max_kp, np.float32) if stereo else None
        n = C.c_int(0)
        self._chk(self.L.drfe_frame_collect(self.h, slot, _p(kps), _p(desc), _p(ur) if stereo else None,
                                            _p(z) if stereo else None, self.max_kp, C.byref(n)), "drfe_frame_collect")
        out = (kps[:n.value].copy(), desc[:n.value].copy())
        return out + (ur[:n.value].copy(), z[:n.value].copy()) if stereo else out

    def frame_submit_tracked(self, slot: int, gray: np.ndarray, depth16: np.ndarray, cam: Camera, last_slot: int, Tcw_cur, Tcw_last,
                             Twc_last=None, last_mp=None, th=15.0, mono=False, check_ori=True):
        """One submission per tracked frame: frame_submit + SearchByProjection(this frame, the frame in last_slot) in the same
        captured graph.  last_mp (MAPPOINT_DTYPE array) = LastFrame.mvpMapPoints; None = its keypoints with depth, unprojected
        with Twc_last on the device."""
        assert gray.dtype == np.uint8 and depth16.dtype == np.uint16 and depth16.shape == gray.shape
        tc = np.ascontiguousarray(Tcw_cur, np.float32); tl = np.ascontiguousarray(Tcw_last, np.float32)
        tw = np.ascontiguousarray(Twc_last, np.float32) if Twc_last is not None else None
        mp = np.ascontiguousarray(last_mp, MAPPOINT_DTYPE) if last_mp is not None else None
        self._chk(self.L.drfe_frame_submit_tracked(self.h, slot, _p(gray), gray.shape[1], gray.shape[0], gray.strides[0], _p(depth16),
                                                   C.c_size_t(depth16.strides[0] // 2), C.byref(cam), last_slot, _p(tc), _p(tl), _p(tw),
                                                   _p(mp), 0 if mp is None else len(mp), float(th), int(mono), int(check_ori)),
                  "drfe_frame_submit_tracked")

    def frame_collect_tracked(self, slot: int):
        """-> (mvKeys, mDescriptors, mvuRight, mvDepth, cur_to_last, nmatches) of the slot's tracked submission."""
        kps = np.zeros(self.max_kp, KP_DTYPE)
        desc = np.zeros((self.max_kp, 32), np.uint8)
        ur = np.zeros(self.max_kp, np.float32); z = np.zeros(self.max_kp, np.float32)
        m = np.full(self.max_kp, -1, np.int32)
        n, nm = C.c_int(0), C.c_int(0)
        self._chk(self.L.drfe_frame_collect_tracked(self.h, slot, _p(kps), _p(desc), _p(ur), _p(z), self.max_kp, C.byref(n), _p(m),
                                                    C.byref(nm)), "drfe_frame_collect_tracked")
        k = n.value
        return kps[:k].copy(), desc[:k].copy(), ur[:k].copy(), z[:k].copy(), m[:k].copy(), nm.value

    def orb_extract_batch_ptr(self, d_gray: int, frame_stride: int, row_stride: int, w: int, h: int, nframes: int,
                              stream: int = 0):
        self._chk(self.L.drfe_orb_extract_batch(self.h, C.c_void_p(d_gray), frame_stride, row_stride, w, h, nframes,
                                                C.c_void_p(stream)), "drfe_orb_extract_batch")

    def orb_download(self, slot: int):
        kps = np.zeros(self.max_kp, KP_DTYPE)
        desc = np.zeros((self.max_kp, 32), np.uint8)
        n = C.c_int(0)
        self._chk(self.L.drfe_orb_download(self.h, slot, _p(kps), _p(desc), self.max_kp, C.byref(n)), "drfe_orb_download")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def batch_download_async_ptr(self, nframes: int, kps: int, desc: int, kp_counts: int, matches: int, match_counts: int,
                                 stream: int = 0):
        """Raw host pointers (pinned torch tensors): see drfe_batch_download_async."""
        self._chk(self.L.drfe_batch_download_async(self.h, nframes, C.c_void_p(kps), C.c_void_p(desc), C.c_void_p(kp_counts),
                                                   C.c_void_p(matches), C.c_void_p(match_counts), C.c_void_p(stream)),
                  "drfe_batch_download_async")

    def fast_partition(self, w: int, h: int):
        """-> (cells[2], evaluated pixels[2]) of the two FAST launches for a w x h frame."""
        cells = np.zeros(2, np.int32)
        px = np.zeros(2, np.int64)
        self._chk(self.L.drfe_orb_fast_partition(self.h, w, h, _p(cells), _p(px)), "drfe_orb_fast_partition")
        return cells, px

    def fast_cells(self, w: int, h: int):
        """-> the FAST cell table of a w x h frame in launch order (FAST_CELL_DTYPE): level, window, offsets, emission index, the
        lane layout of k_fast_cells_cols, the kernel each cell runs (8 / 12, 0 = the generic k_fast_cells) and the survivor-list
        capacity of that launch.  Host code."""
        n = C.c_int(0)
        self._chk(self.L.drfe_orb_fast_cells(self.h, w, h, None, 0, C.byref(n)), "drfe_orb_fast_cells")
        rows = np.zeros(max(n.value, 1), FAST_CELL_DTYPE)
        self._chk(self.L.drfe_orb_fast_cells(self.h, w, h, _p(rows), len(rows), C.byref(n)), "drfe_orb_fast_cells")
        return rows[:n.value]

    def orb_counts(self, nframes: int):
        c = np.zeros(nframes, np.int32)
        self._chk(self.L.drfe_orb_counts(self.h, nframes, _p(c)), "drfe_orb_counts")
        return c

    def orb_configure_level0(self, in_place=True):
        """Whether orb_extract_batch_ptr may read pyramid level 0 from the caller's frames (default) or always copies it."""
        self._chk(self.L.drfe_orb_configure_level0(self.h, 1 if in_place else 0), "drfe_orb_configure_level0")

    def orb_level0_in_place(self) -> bool:
        """True if the most recent batch read pyramid level 0 in place."""
        rc = self.L.drfe_orb_level0_in_place(self.h)
        self._chk(min(rc, 0), "drfe_orb_level0_in_place")
        return rc == 1

    def pyramid_level(self, slot, level):
        w, h = C.c_int(), C.c_int()
        self._chk(self.L.drfe_orb_pyramid_level(self.h, slot, level, None, C.byref(w), C.byref(h)), "pyramid_level")
        out = np.zeros((h.value, w.value), np.uint8)
        self._chk(self.L.drfe_orb_pyramid_level(self.h, slot, level, _p(out), C.byref(w), C.byref(h)), "pyramid_level")
        return out

    def blurred_level(self, slot, level):
        w, h = C.c_int(), C.c_int()
        self._chk(self.L.drfe_orb_blurred_level(self.h, slot, level, None, C.byref(w), C.byref(h)), "blurred_level")
        out = np.zeros((h.value, w.value), np.uint8)
        self._chk(self.L.drfe_orb_blurred_level(self.h, slot, level, _p(out), C.byref(w), C.byref(h)), "blurred_level")
        return out

    def candidates(self, slot, level):
        n = C.c_int()
        self._chk(self.L.drfe_orb_candidates(self.h, slot, level, None, 0, C.byref(n)), "candidates")
        out = np.zeros((max(n.value, 1), 3), np.int32)
        self._chk(self.L.drfe_orb_candidates(self.h, slot, level, _p(out), len(out), C.byref(n)), "candidates")
        return out[:n.value]

    # --- Frame glue --------------------------------------------------------------------------------
    def stereo_grid_batch_ptr(self, d_depth: int, frame_stride_elems: int, row_stride_elems: int, cam: Camera,
                              nframes: int, stream: int = 0):
        self._chk(self.L.drfe_frame_stereo_grid_batch(self.h, C.c_void_p(d_depth), frame_stride_elems,
                                                      row_stride_elems, C.byref(cam), nframes, C.c_void_p(stream)),
                  "drfe_frame_stereo_grid_batch")

    def keypoint_pixels_async_ptr(self, nframes: int, uv: int, counts: int, stream: int = 0):
        """uv / counts: raw host pointers (pinned) of [nframes][max_kp] uint32 and [nframes] int32."""
        self._chk(self.L.drfe_orb_keypoint_pixels_async(self.h, nframes, C.c_void_p(uv), C.c_void_p(counts), C.c_void_p(stream)),
                  "drfe_orb_keypoint_pixels_async")

    def gather_keypoint_depth(self, depth16: np.ndarray, uv: np.ndarray, counts: np.ndarray, out: np.ndarray, n_threads=0):
        """Host gather: out[f, i] = depth16[f, v, u] for the pixels drfe_orb_keypoint_pixels_async reported."""
        B, h, w = depth16.shape
        rc = self.L.drfe_gather_keypoint_depth(_p(depth16), w * h, w, B, _p(uv), _p(counts), self.max_kp, _p(out), int(n_threads))
        if rc != 0:
            raise DrfeError(f"drfe_gather_keypoint_depth failed ({rc})")

    def stereo_grid_batch_kpdepth_ptr(self, kp_depth: int, on_host: bool, cam: Camera, nframes: int, stream: int = 0):
        self._chk(self.L.drfe_frame_stereo_grid_batch_kpdepth(self.h, C.c_void_p(kp_depth), int(on_host), C.byref(cam), nframes,
                                                               C.c_void_p(stream)), "drfe_frame_stereo_grid_batch_kpdepth")

    def download_stereo(self, slot):
        ur = np.zeros(self.max_kp, np.float32)
        z = np.zeros(self.max_kp, np.float32)
        self._chk(self.L.drfe_frame_download_stereo(self.h, slot, _p(ur), _p(z), self.max_kp), "download_stereo")
        return ur, z

    def frame_load(self, slot, kps, desc, cam: Camera, kps_un=None, u_right=None, depth_m=None):
        """drfe_frame_load: a host-held frame (KeyFrame members mvKeys / mvKeysUn / mDescriptors / mvuRight / mvDepth) into `slot`;
        the 64 x 48 grid is rebuilt on the device."""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(kps)
        ku = None if kps_un is None else np.ascontiguousarray(kps_un, KP_DTYPE)
        ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        z = None if depth_m is None else np.ascontiguousarray(depth_m, np.float32)
        self._chk(self.L.drfe_frame_load(self.h, slot, _p(kps), _p(ku), _p(desc), _p(ur), _p(z), n, C.byref(cam)), "drfe_frame_load")

    def download_grid(self, slot):
        off = np.zeros(64 * 48 + 1, np.int32)
        idx = np.zeros(self.max_kp, np.int32)
        self._chk(self.L.drfe_frame_download_grid(self.h, slot, _p(off), _p(idx), self.max_kp), "download_grid")
        return off, idx[:off[-1]].copy()

    # --- matchers ----------------------------------------------------------------------------------
    def match_consecutive_batch(self, Tcw: np.ndarray, Twc: np.ndarray, cam: Camera, th=15.0, mono=False,
                                check_ori=True, nframes=None, stream: int = 0):
        Tcw = np.ascontiguousarray(Tcw, np.float32)
        Twc = np.ascontiguousarray(Twc, np.float32)
        nframes = len(Tcw) if nframes is None else nframes
        self._chk(self.L.drfe_match_consecutive_batch(self.h, _p(Tcw), _p(Twc), C.byref(cam), th, int(mono),
                                                      int(check_ori), nframes, C.c_void_p(stream)),
                  "drfe_match_consecutive_batch")

    def match_download(self, slot):
        m = np.zeros(self.max_kp, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_match_download(self.h, slot, _p(m), self.max_kp, C.byref(n)), "drfe_match_download")
        return m, n.value

    def search_by_projection_last(self, cur_slot, last_slot, Tcw_cur, Tcw_last, cam, last_mp, n_cur, th=15.0,
                                  mono=False, check_ori=True, cur_mp=None, cur_obs=None):
        last_mp = np.ascontiguousarray(last_mp, MAPPOINT_DTYPE)
        out = np.full(n_cur, -1, np.int32) if cur_mp is None else np.ascontiguousarray(cur_mp, np.int32).copy()
        obs = None if cur_obs is None else np.ascontiguousarray(cur_obs, np.uint8)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_projection_last(
            self.h, cur_slot, last_slot, _p(np.ascontiguousarray(Tcw_cur, np.float32)),
            _p(np.ascontiguousarray(Tcw_last, np.float32)), C.byref(cam), _p(last_mp), len(last_mp), th, int(mono),
            int(check_ori), _p(obs), _p(out), n_cur, C.byref(n)), "drfe_search_by_projection_last")
        return n.value, out

    def search_by_projection_map(self, slot, mps, n, th, nnratio, frame_mp=None, claim_obs=None):
        mps = np.ascontiguousarray(mps, TRACKED_DTYPE)
        out = np.full(n, -1, np.int32) if frame_mp is None else np.ascontiguousarray(frame_mp, np.int32).copy()
        obs = None if claim_obs is None else np.ascontiguousarray(claim_obs, np.uint8)
        nm = C.c_int()
        self._chk(self.L.drfe_search_by_projection_map(self.h, slot, _p(mps), len(mps), th, nnratio, _p(obs), _p(out),
                                                       n, C.byref(nm)), "drfe_search_by_projection_map")
        return nm.value, out

    def match_orb_points(self, cur_slot, last_slot, last_mp, last_outlier, n_cur, cur_mp=None):
        last_mp = np.ascontiguousarray(last_mp, np.int32)
        last_outlier = np.ascontiguousarray(last_outlier, np.uint8)
        out = np.full(n_cur, -1, np.int32) if cur_mp is None else np.ascontiguousarray(cur_mp, np.int32).copy()
        n = C.c_int()
        self._chk(self.L.drfe_match_orb_points(self.h, cur_slot, last_slot, _p(last_mp), _p(last_outlier), len(last_mp),
                                               _p(out), n_cur, C.byref(n)), "drfe_match_orb_points")
        return n.value, out

    def is_in_frustum(self, Tcw, cam, pts, viewing_cos_limit, out=None):
        """Frame::isInFrustum(MapPoint*, limit) for an array of map points; returns the drfe_tracked_point array with
        the tracking fields filled (bad / obs_positive / desc of `out` are preserved)."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        p = np.ascontiguousarray(pts, FRUSTUM_POINT_DTYPE)
        o = np.zeros(len(p), TRACKED_DTYPE) if out is None else np.ascontiguousarray(out, TRACKED_DTYPE).copy()
        self._chk(self.L.drfe_frame_is_in_frustum(self.h, _p(T), C.byref(cam), _p(p), len(p), C.c_float(viewing_cos_limit),
                                                  _p(o)), "drfe_frame_is_in_frustum")
        return o

    def fuse_search(self, slot, Tcw, pts, descs, skip, th):
        """Search part of ORBmatcher::Fuse(pKF, vpMapPoints, th); returns (best_idx, best_dist) per map point."""
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        p = np.ascontiguousarray(pts, FRUSTUM_POINT_DTYPE)
        d = np.ascontiguousarray(descs, np.uint8)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        bi = np.zeros(len(p), np.int32)
        bd = np.zeros(len(p), np.int32)
        self._chk(self.L.drfe_fuse_search(self.h, slot, _p(T), _p(p), _p(d), _p(sk), len(p), C.c_float(th), _p(bi), _p(bd)),
                  "drfe_fuse_search")
        return bi, bd

    def fuse_search_sim3(self, slot, Scw, pts, descs, skip, th):
        """Search part of ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)."""
        T = np.ascontiguousarray(Scw, np.float32).reshape(16)
        p = np.ascontiguousarray(pts, FRUSTUM_POINT_DTYPE)
        d = np.ascontiguousarray(descs, np.uint8)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        bi = np.zeros(len(p), np.int32)
        bd = np.zeros(len(p), np.int32)
        self._chk(self.L.drfe_fuse_search_sim3(self.h, slot, _p(T), _p(p), _p(d), _p(sk), len(p), C.c_float(th), _p(bi), _p(bd)),
                  "drfe_fuse_search_sim3")
        return bi, bd

    def lsd_fuse_search(self, Tcw, cam, lines, descs, skip, kf_lines, kf_desc, th):
        """Search part of LSDmatcher::Fuse(pKF, vpMapLines, th); returns (best_idx, best_dist) per map line."""
        l = np.ascontiguousarray(lines, FRUSTUM_LINE_DTYPE)
        kl = np.ascontiguousarray(kf_lines, KEYLINE_DTYPE)
        bi = np.zeros(len(l), np.int32)
        bd = np.zeros(len(l), np.int32)
        self._chk(self.L.drfe_lsd_fuse_search(self.h, _p(np.ascontiguousarray(Tcw, np.float32).reshape(16)), C.byref(cam), _p(l),
                                              _p(np.ascontiguousarray(descs, np.uint8)), _p(np.ascontiguousarray(skip, np.uint8)),
                                              len(l), _p(kl), _p(np.ascontiguousarray(kf_desc, np.uint8)), len(kl), C.c_float(th),
                                              _p(bi), _p(bd)), "drfe_lsd_fuse_search")
        return bi, bd

    def lsd_fuse_search_sim3(self, Scw, cam, lines, descs, skip, kf_lines, kf_desc, th):
        """Search part of LSDmatcher::Fuse(pKF, Scw, vpLines, th, vpReplaceLine); returns (best_idx, best_dist) per map line."""
        l = np.ascontiguousarray(lines, FRUSTUM_LINE_DTYPE)
        kl = np.ascontiguousarray(kf_lines, KEYLINE_DTYPE)
        bi = np.zeros(len(l), np.int32)
        bd = np.zeros(len(l), np.int32)
        self._chk(self.L.drfe_lsd_fuse_search_sim3(self.h, _p(np.ascontiguousarray(Scw, np.float32).reshape(16)), C.byref(cam), _p(l),
                                                   _p(np.ascontiguousarray(descs, np.uint8)), _p(np.ascontiguousarray(skip, np.uint8)),
                                                   len(l), _p(kl), _p(np.ascontiguousarray(kf_desc, np.uint8)), len(kl), C.c_float(th),
                                                   _p(bi), _p(bd)), "drfe_lsd_fuse_search_sim3")
        return bi, bd

    def lsd_search_by_projection_kf(self, Scw, cam, lines, descs, skip, kf_lines, kf_desc, matched, th):
        """LSDmatcher::SearchByProjection(pKF, Scw, vpLines, vpMatched, th); returns (nmatches, new_match per key line)."""
        l = np.ascontiguousarray(lines, FRUSTUM_LINE_DTYPE)
        kl = np.ascontiguousarray(kf_lines, KEYLINE_DTYPE)
        m = np.ascontiguousarray(matched, np.uint8)
        out = np.full(len(kl), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_by_projection_kf(self.h, _p(np.ascontiguousarray(Scw, np.float32).reshape(16)), C.byref(cam),
                                                          _p(l), _p(np.ascontiguousarray(descs, np.uint8)),
                                                          _p(np.ascontiguousarray(skip, np.uint8)), len(l), _p(kl),
                                                          _p(np.ascontiguousarray(kf_desc, np.uint8)), len(kl), _p(m), int(th), _p(out),
                                                          C.byref(n)), "drfe_lsd_search_by_projection_kf")
        return n.value, out

    def lsd_search_by_sim3(self, cam, T1w, T2w, s12, R12, t12, lines1, descs1, skip1, kf1_lines, kf1_desc, lines2, descs2, skip2,
                           kf2_lines, kf2_desc, th):
        """LSDmatcher::SearchBySim3; returns (nFound, matches12[i1] = key line of KF2 or -1)."""
        f = lambda a, n: _p(np.ascontiguousarray(a, np.float32).reshape(n))
        u8 = lambda a: _p(np.ascontiguousarray(a, np.uint8))
        l1, l2 = np.ascontiguousarray(lines1, FRUSTUM_LINE_DTYPE), np.ascontiguousarray(lines2, FRUSTUM_LINE_DTYPE)
        k1, k2 = np.ascontiguousarray(kf1_lines, KEYLINE_DTYPE), np.ascontiguousarray(kf2_lines, KEYLINE_DTYPE)
        assert len(l1) == len(k1) and len(l2) == len(k2)
        out = np.full(len(l1), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_by_sim3(self.h, C.byref(cam), f(T1w, 16), f(T2w, 16), C.c_float(s12), f(R12, 9), f(t12, 3),
                                                 _p(l1), u8(descs1), u8(skip1), _p(k1), u8(kf1_desc), len(l1), _p(l2), u8(descs2),
                                                 u8(skip2), _p(k2), u8(kf2_desc), len(l2), C.c_float(th), _p(out), C.byref(n)),
                  "drfe_lsd_search_by_sim3")
        return n.value, out

    def search_by_projection_kf(self, slot, Scw, pts, descs, skip, matched, th):
        """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th); returns (nmatches, new_match per keypoint)."""
        p = np.ascontiguousarray(pts, FRUSTUM_POINT_DTYPE)
        m = np.ascontiguousarray(matched, np.uint8)
        out = np.full(len(m), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_projection_kf(self.h, slot, _p(np.ascontiguousarray(Scw, np.float32).reshape(16)), _p(p),
                                                      _p(np.ascontiguousarray(descs, np.uint8)),
                                                      _p(np.ascontiguousarray(skip, np.uint8)), len(p), _p(m), len(m),
                                                      C.c_float(th), _p(out), C.byref(n)), "drfe_search_by_projection_kf")
        return n.value, out

    def search_by_projection_reloc(self, slot, Tcw, pts, descs, kf_angles, skip, matched, th, orb_dist, check_orientation=True):
        """ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist); returns (nmatches, new_match)."""
        p = np.ascontiguousarray(pts, FRUSTUM_POINT_DTYPE)
        m = np.ascontiguousarray(matched, np.uint8)
        out = np.full(len(m), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_projection_reloc(self.h, slot, _p(np.ascontiguousarray(Tcw, np.float32).reshape(16)), _p(p),
                                                         _p(np.ascontiguousarray(descs, np.uint8)),
                                                         _p(np.ascontiguousarray(kf_angles, np.float32)),
                                                         _p(np.ascontiguousarray(skip, np.uint8)), len(p), _p(m), len(m),
                                                         C.c_float(th), int(orb_dist), int(bool(check_orientation)), _p(out),
                                                         C.byref(n)), "drfe_search_by_projection_reloc")
        return n.value, out

    def search_for_initialization(self, slot1, slot2, prev_matched, window_size=100, nnratio=0.9, check_orientation=True):
        """ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize); returns (nmatches, matches12,
        prev_matched after the update)."""
        pm = np.ascontiguousarray(prev_matched, np.float32).reshape(-1, 2).copy()
        out = np.full(len(pm), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_for_initialization(self.h, slot1, slot2, _p(pm), len(pm), int(window_size), C.c_float(nnratio),
                                                        int(bool(check_orientation)), _p(out), C.byref(n)),
                  "drfe_search_for_initialization")
        return n.value, out, pm

    def search_by_sim3(self, slot1, slot2, T1w, T2w, s12, R12, t12, pts1, descs1, skip1, pts2, descs2, skip2, th):
        """ORBmatcher::SearchBySim3; returns (nFound, matches12[i1] = i2 or -1)."""
        f = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
        p1, p2 = np.ascontiguousarray(pts1, FRUSTUM_POINT_DTYPE), np.ascontiguousarray(pts2, FRUSTUM_POINT_DTYPE)
        out = np.full(len(p1), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_sim3(self.h, slot1, slot2, _p(f(T1w, 16)), _p(f(T2w, 16)), C.c_float(s12), _p(f(R12, 9)),
                                             _p(f(t12, 3)), _p(p1), _p(np.ascontiguousarray(descs1, np.uint8)),
                                             _p(np.ascontiguousarray(skip1, np.uint8)), len(p1), _p(p2),
                                             _p(np.ascontiguousarray(descs2, np.uint8)), _p(np.ascontiguousarray(skip2, np.uint8)),
                                             len(p2), C.c_float(th), _p(out), C.byref(n)), "drfe_search_by_sim3")
        return n.value, out

    def is_in_frustum_lines(self, Tcw, cam, lines, viewing_cos_limit, out=None):
        T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
        l = np.ascontiguousarray(lines, FRUSTUM_LINE_DTYPE)
        o = np.zeros(len(l), TRACKED_LINE_DTYPE) if out is None else np.ascontiguousarray(out, TRACKED_LINE_DTYPE).copy()
        self._chk(self.L.drfe_frame_is_in_frustum_lines(self.h, _p(T), C.byref(cam), _p(l), len(l),
                                                        C.c_float(viewing_cos_limit), _p(o)), "drfe_frame_is_in_frustum_lines")
        return o

    def set_distortion(self, cam, dist):
        """Frame::UndistortKeyPoints model (k1, k2, p1, p2[, k3]); None / k1 == 0 switches it off."""
        d = np.zeros(0, np.float32) if dist is None else np.ascontiguousarray(dist, np.float32)
        self._chk(self.L.drfe_frame_set_distortion(self.h, C.byref(cam), _p(d), len(d)), "drfe_frame_set_distortion")

    def image_bounds(self, cam, dist, cols, rows):
        d = np.zeros(0, np.float32) if dist is None else np.ascontiguousarray(dist, np.float32)
        out = np.zeros(4, np.float32)
        self._chk(self.L.drfe_frame_image_bounds(C.byref(cam), _p(d), len(d), int(cols), int(rows), _p(out)),
                  "drfe_frame_image_bounds")
        return out

    def download_keys_un(self, slot, n):
        out = np.zeros(max(n, 1), KP_DTYPE)
        self._chk(self.L.drfe_frame_download_keys_un(self.h, slot, _p(out), len(out)), "drfe_frame_download_keys_un")
        return out[:n]

    def lsd_search_by_descriptor(self, desc_q, desc_t, has_line=None, mode=0):
        dq = np.ascontiguousarray(desc_q, np.uint8)
        dt = np.ascontiguousarray(desc_t, np.uint8)
        has = None if has_line is None else np.ascontiguousarray(has_line, np.uint8)
        out = np.full(len(dt) if mode == 0 else len(dq), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_by_descriptor(self.h, _p(dq), len(dq), _p(dt), len(dt), _p(has), mode, _p(out),
                                                       C.byref(n)), "drfe_lsd_search_by_descriptor")
        return n.value, out

    def lsd_search_by_projection_last(self, Tcw_cur, Tcw_last, cam, last_lines, cur_lines, cur_desc, th, mono, nnratio,
                                      cur_ml, cur_obs=None):
        """LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono); returns (nmatches, cur_ml)."""
        tc = np.ascontiguousarray(Tcw_cur, np.float32).reshape(16)
        tl = np.ascontiguousarray(Tcw_last, np.float32).reshape(16)
        ll = np.ascontiguousarray(last_lines, MAPLINE_DTYPE)
        kl = np.ascontiguousarray(cur_lines, KEYLINE_DTYPE)
        cd = np.ascontiguousarray(cur_desc, np.uint8)
        out = np.ascontiguousarray(cur_ml, np.int32).copy()
        obs = None if cur_obs is None else np.ascontiguousarray(cur_obs, np.uint8)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_by_projection_last(self.h, _p(tc), _p(tl), C.byref(cam), _p(ll), len(ll), _p(kl),
                                                            _p(cd), len(kl), C.c_float(th), int(mono), C.c_float(nnratio),
                                                            _p(obs), _p(out), C.byref(n)),
                  "drfe_lsd_search_by_projection_last")
        return n.value, out

    def lsd_search_by_projection_map(self, lines, cur_lines, cur_desc, th, nnratio, cur_ml, cur_obs=None):
        """LSDmatcher::SearchByProjection(F, vpMapLines, th); returns (nmatches, cur_ml)."""
        tl = np.ascontiguousarray(lines, TRACKED_LINE_DTYPE)
        kl = np.ascontiguousarray(cur_lines, KEYLINE_DTYPE)
        cd = np.ascontiguousarray(cur_desc, np.uint8)
        out = np.ascontiguousarray(cur_ml, np.int32).copy()
        obs = None if cur_obs is None else np.ascontiguousarray(cur_obs, np.uint8)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_by_projection_map(self.h, _p(tl), len(tl), _p(kl), _p(cd), len(kl), C.c_float(th),
                                                           C.c_float(nnratio), _p(obs), _p(out), C.byref(n)),
                  "drfe_lsd_search_by_projection_map")
        return n.value, out

    def lsd_search_for_triangulation(self, desc1, desc2, has1, has2):
        d1 = np.ascontiguousarray(desc1, np.uint8)
        d2 = np.ascontiguousarray(desc2, np.uint8)
        out = np.full(len(d1), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_lsd_search_for_triangulation(self.h, _p(d1), len(d1), _p(d2), len(d2),
                                                           _p(np.ascontiguousarray(has1, np.uint8)),
                                                           _p(np.ascontiguousarray(has2, np.uint8)), _p(out), C.byref(n)),
                  "drfe_lsd_search_for_triangulation")
        return n.value, out

    def bf_knn(self, Q, T, k):
        Q = np.ascontiguousarray(Q, np.uint8)
        T = np.ascontiguousarray(T, np.uint8)
        idx = np.zeros((len(Q), k), np.int32)
        dist = np.zeros((len(Q), k), np.int32)
        self._chk(self.L.drfe_match_bf_knn(self.h, _p(Q), len(Q), _p(T), len(T), k, _p(idx), _p(dist)), "drfe_match_bf_knn")
        return idx, dist

    # --- lines -------------------------------------------------------------------------------------
    def lsd_extract(self, gray: np.ndarray, max_lines=40, stages=False):
        """LineSegment::ExtractLineSegment -> dict(lines, desc, lineF, detected[, stage images])."""
        g = np.ascontiguousarray(gray, np.uint8)
        h, w = g.shape
        cap = max_lines
        lines = np.zeros(cap, KEYLINE_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        lf = np.zeros((cap, 3))
        n, nd = C.c_int(), C.c_int()
        self._chk(self.L.drfe_lsd_extract(self.h, _p(g), w, h, w, max_lines, _p(lines), _p(desc), _p(lf), cap,
                                          C.byref(n), C.byref(nd)), "drfe_lsd_extract")
        out = dict(lines=lines[:n.value].copy(), desc=desc[:n.value].copy(), lineF=lf[:n.value].copy(), detected=nd.value)
        if stages:
            sw, sh = C.c_int(), C.c_int()
            self._chk(self.L.drfe_lsd_stages(self.h, None, None, None, None, None, C.byref(sw), C.byref(sh)), "lsd_stages")
            scaled = np.zeros((sh.value, sw.value), np.uint8)
            modgrad, angles = np.zeros((sh.value, sw.value)), np.zeros((sh.value, sw.value))
            gx, gy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
            self._chk(self.L.drfe_lsd_stages(self.h, _p(scaled), _p(modgrad), _p(angles), _p(gx), _p(gy), C.byref(sw),
                                             C.byref(sh)), "lsd_stages")
            out.update(scaled=scaled, modgrad=modgrad, angles=angles, gx=gx, gy=gy)
        return out

    def lsd_configure(self, device_grow=True):
        """Where lsd_extract_batch grows its regions: False / 0 the host pool; True / 1 the device, kernel chosen by the size of the
        call (default); 2 the device with one wavefront per frame; 3 with four (speculation + in-order commit)."""
        self._chk(self.L.drfe_lsd_configure(self.h, int(device_grow)), "drfe_lsd_configure")

    def planes_configure_cape(self, on_device=True):
        """Where planes_cape_batch runs CAPE::process (histogram seeding, cell growing, merging, masks): device or host pool."""
        self._chk(self.L.drfe_planes_configure_cape(self.h, 1 if on_device else 0), "drfe_planes_configure_cape")

    def planes_ahc_stats(self):
        """dict(frames, to_host, voxel_grids, voxel_grids_to_host): counters of the device extractor behind planes_ahc_batch /
        planes_ahc_post_batch since the context was created"""
        out = np.zeros(4, np.int64)
        self._chk(self.L.drfe_planes_ahc_stats(self.h, _p(out)), "drfe_planes_ahc_stats")
        return dict(frames=int(out[0]), to_host=int(out[1]), voxel_grids=int(out[2]), voxel_grids_to_host=int(out[3]))

    def planes_configure_refit(self, on_device=True):
        """Where planes_ahc_post_batch runs gates + RANSAC refit: the device behind the device voxel grids (default) or the host pool."""
        self._chk(self.L.drfe_planes_configure_refit(self.h, 1 if on_device else 0), "drfe_planes_configure_refit")

    def debug_device_voxel_grid(self, clouds, leaf=0.05, depth_limit=-1, workgroups=0, recs=True):
        """Test hook: up to 256 [n, 3] float32 clouds through one device voxel-grid lane (k_voxel_jobs_order + k_voxel_grid) ->
        (counts [n_clouds] as the kernel wrote them: >= 0 centroids, -1 grid beyond int32, -2 heap-sort hand-back, <= -9 a loop
        bound; centroids: list of [count, 3] arrays, empty where count <= 0; records: list of the sorted leaf << 32 | point uint64
        arrays, or None)."""
        xyz, off = _csr(clouds)
        out = np.zeros_like(xyz)
        counts = np.zeros(len(clouds), np.int32)
        rec = np.zeros(len(xyz), np.uint64) if recs else None
        self._chk(self.L.drfe_debug_device_voxel_grid(self.h, _p(xyz), _p(off), len(clouds), np.float32(leaf), depth_limit, workgroups, _p(out), _p(counts),
                                                      _p(rec) if recs else None), "drfe_debug_device_voxel_grid")
        cent = [out[off[i]:off[i] + max(0, int(counts[i]))].copy() for i in range(len(clouds))]
        return counts, cent, ([rec[off[i]:off[i + 1]].copy() for i in range(len(clouds))] if recs else None)

    def planes_refit_stats(self):
        out = np.zeros(2, np.int64)
        self._chk(self.L.drfe_planes_refit_stats(self.h, _p(out)), "drfe_planes_refit_stats")
        return dict(frames=int(out[0]), to_host=int(out[1]))

    def planes_cape_stats(self):
        out = np.zeros(2, np.int64)
        self._chk(self.L.drfe_planes_cape_stats(self.h, _p(out)), "drfe_planes_cape_stats")
        return dict(frames=int(out[0]), to_host=int(out[1]))

    def lsd_configure_nfa(self, device_nfa=True):
        """Where lsd_extract_batch takes rect_improve's NFA decisions: on the device (certified comparisons, default) or on the
        host pool with the caller's libm."""
        self._chk(self.L.drfe_lsd_configure_nfa(self.h, 1 if device_nfa else 0), "drfe_lsd_configure_nfa")

    def long_kernel_clock(self, on=True):
        """lsd_extract_batch / planes_ahc_post_batch bracket every kernel of their first chunk with HIP events (long_kernel_ms)"""
        self._chk(self.L.drfe_long_kernel_clock(self.h, int(bool(on))), "drfe_long_kernel_clock")

    def long_kernel_ms(self):
        """ms of the last clocked batch call's first chunk, by kernel (0 where the stage ran elsewhere)"""
        out = np.zeros(16, np.float32)
        self._chk(self.L.drfe_long_kernel_ms(self.h, _p(out)), "drfe_long_kernel_ms")
        names = ("lines_upload", "lines_image_passes", "k_lsd_keys", "k_lsd_order", "k_lsd_grow", "k_rect_improve", "k_lsd_keylines+k_lbd", None,
                 "planes_upload", "k_ahc_blocks", "k_ahc_cluster", "k_ahc_refine", "k_ahc_labels", "k_voxel_grid", "k_plane_refit", None)
        return {n: float(v) for n, v in zip(names, out) if n}

    def lsd_stats(self):
        """dict(frames, grow_to_host, nfa_to_host, keylines_to_host): counters of lsd_extract_batch's device path since the context was created"""
        out = np.zeros(4, np.int64)
        self._chk(self.L.drfe_lsd_stats(self.h, _p(out)), "drfe_lsd_stats")
        return dict(frames=int(out[0]), grow_to_host=int(out[1]), nfa_to_host=int(out[2]), keylines_to_host=int(out[3]))

    def lsd_configure_rect(self, rect_mode=0):
        """The reading of OpenCV 3.4's lsd.cpp: 0 the source text (rect_nfa's integer corners and step quotients, nfa()'s
        `double(n) + 1` first term; default), 1 the LSD paper's reading of both (rounds 2-3), 2 integer corners with
        log_gamma(n + 1) (round 4's default)."""
        self._chk(self.L.drfe_lsd_configure_rect(self.h, int(rect_mode)), "drfe_lsd_configure_rect")

    def lsd_extract_batch(self, gray_batch: np.ndarray, max_lines=40, n_threads=0):
        """LineSegment::ExtractLineSegment for a [B, H, W] uint8 host array: region growing on the device (or, after
        lsd_configure(False), on the host pool), ordering + NFA on a pool of host threads; returns a list of dicts like
        lsd_extract."""
        g = np.ascontiguousarray(gray_batch, np.uint8)
        B, h, w = g.shape
        cap = max_lines
        lines = np.zeros((B, cap), KEYLINE_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        lf = np.zeros((B, cap, 3))
        n = np.zeros(B, np.int32)
        nd = np.zeros(B, np.int32)
        self._chk(self.L.drfe_lsd_extract_batch(self.h, _p(g), w * h, w, h, w, B, max_lines, _p(lines), _p(desc), _p(lf), cap,
                                                _p(n), _p(nd), int(n_threads)), "drfe_lsd_extract_batch")
        return [dict(lines=lines[f, :n[f]].copy(), desc=desc[f, :n[f]].copy(), lineF=lf[f, :n[f]].copy(), detected=int(nd[f]))
                for f in range(B)]

    # --- bag of words ------------------------------------------------------------------------------
    def voc_upload(self, k, L, scoring, weighting, parent, desc, weight, is_leaf):
        parent = np.ascontiguousarray(parent, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        weight = np.ascontiguousarray(weight, np.float64)
        is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        self._chk(self.L.drfe_voc_upload(self.h, k, L, scoring, weighting, len(parent), _p(parent), _p(desc), _p(weight),
                                         _p(is_leaf)), "drfe_voc_upload")

    def bow_transform_batch(self, levelsup, nframes, stream: int = 0):
        self._chk(self.L.drfe_bow_transform_batch(self.h, levelsup, nframes, C.c_void_p(stream)), "drfe_bow_transform_batch")

    def bow_transform_slot(self, levelsup, slot, stream: int = 0):
        self._chk(self.L.drfe_bow_transform_slot(self.h, levelsup, slot, C.c_void_p(stream)), "drfe_bow_transform_slot")

    def bow_download(self, slot):
        word = np.zeros(self.max_kp, np.int32)
        weight = np.zeros(self.max_kp, np.float64)
        nid = np.zeros(self.max_kp, np.int32)
        self._chk(self.L.drfe_bow_download(self.h, slot, _p(word), _p(weight), _p(nid), self.max_kp), "drfe_bow_download")
        return word, weight, nid

    def search_by_bow(self, kf_slot, f_slot, kf_mp, n_f, nnratio, check_ori=True):
        kf_mp = np.ascontiguousarray(kf_mp, np.int32)
        out = np.full(n_f, -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_bow(self.h, kf_slot, f_slot, _p(kf_mp), len(kf_mp), nnratio, int(check_ori),
                                            _p(out), n_f, C.byref(n)), "drfe_search_by_bow")
        return n.value, out

    def search_by_bow_kf(self, slot1, slot2, mp1, mp2, nnratio, check_ori=True):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12); returns (nmatches, match2) with match2[i2] = i1 or -1."""
        mp1 = np.ascontiguousarray(mp1, np.int32)
        mp2 = np.ascontiguousarray(mp2, np.int32)
        out = np.full(len(mp2), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_by_bow_kf(self.h, slot1, slot2, _p(mp1), len(mp1), _p(mp2), len(mp2), C.c_float(nnratio),
                                               int(check_ori), _p(out), C.byref(n)), "drfe_search_by_bow_kf")
        return n.value, out

    def search_for_triangulation(self, slot1, slot2, mp1, mp2, F12, Cw1, T2w, cam2, only_stereo=False, check_ori=True):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, pairs, bOnlyStereo); returns (nmatches, matches12)."""
        mp1 = np.ascontiguousarray(mp1, np.int32)
        mp2 = np.ascontiguousarray(mp2, np.int32)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        Cw = np.ascontiguousarray(Cw1, np.float32).reshape(3)
        T = np.ascontiguousarray(T2w, np.float32).reshape(16)
        out = np.full(len(mp1), -1, np.int32)
        n = C.c_int()
        self._chk(self.L.drfe_search_for_triangulation(self.h, slot1, slot2, _p(mp1), len(mp1), _p(mp2), len(mp2), _p(F), _p(Cw),
                                                       _p(T), C.byref(cam2), int(only_stereo), int(check_ori), _p(out),
                                                       C.byref(n)), "drfe_search_for_triangulation")
        return n.value, out

    # --- planes ------------------------------------------------------------------------------------
    def planes_ahc(self, depth16: np.ndarray, K4, depth_factor, cap=64):
        """PlaneDetection::readDepthImage + runPlaneDetection -> dict(planes, seg, members)."""
        d = np.ascontiguousarray(depth16, np.uint16)
        h, w = d.shape
        K4 = np.ascontiguousarray(K4, np.float32)
        planes = np.zeros(cap, PLANE_DTYPE)
        n = C.c_int()
        seg = np.zeros((h, w), np.uint8)
        off = np.zeros(cap + 1, np.int32)
        idx = np.zeros(h * w, np.int32)
        self._chk(self.L.drfe_planes_ahc(self.h, _p(d), w, h, w, _p(K4), np.float32(depth_factor), _p(planes), cap,
                                         C.byref(n), _p(seg), _p(off), _p(idx)), "drfe_planes_ahc")
        n = n.value
        return dict(planes=planes[:n].copy(), seg=seg, members=[idx[off[i]:off[i + 1]].copy() for i in range(n)])

    def planes_ahc_batch(self, depth16_batch: np.ndarray, K4, depth_factor, cap=64, n_threads=0, members=True):
        """drfe_planes_ahc for a [B, H, W] uint16 host array on a pool of host threads; list of dicts like planes_ahc."""
        d = np.ascontiguousarray(depth16_batch, np.uint16)
        B, h, w = d.shape
        K4 = np.ascontiguousarray(K4, np.float32)
        planes = np.zeros((B, cap), PLANE_DTYPE)
        n = np.zeros(B, np.int32)
        seg = np.zeros((B, h, w), np.uint8)
        off = np.zeros((B, cap + 1), np.int32) if members else None
        idx = np.zeros((B, h * w), np.int32) if members else None
        self._chk(self.L.drfe_planes_ahc_batch(self.h, _p(d), w * h, w, h, w, B, _p(K4), np.float32(depth_factor), _p(planes),
                                               cap, _p(n), _p(seg), _p(off), _p(idx), int(n_threads)), "drfe_planes_ahc_batch")
        out = []
        for f in range(B):
            r = dict(planes=planes[f, :n[f]].copy(), seg=seg[f])
            if members:
                r["members"] = [idx[f, off[f, i]:off[f, i + 1]].copy() for i in range(n[f])]
            out.append(r)
        return out

    def planes_configure(self, device_voxel_grid=1):
        """Where planes_ahc_post_batch runs the per-plane voxel grids: 1 (default) the device behind the device extractor, 2 the
        device in the host-extractor mode too, 0 the pool's host threads."""
        self._chk(self.L.drfe_planes_configure(self.h, int(device_voxel_grid)), "drfe_planes_configure")

    def planes_configure_extractor(self, on_device=True):
        """Where planes_ahc_post_batch runs PEAC's extractor: the device (one wavefront per frame, default) or the host pool."""
        self._chk(self.L.drfe_planes_configure_extractor(self.h, 1 if on_device else 0), "drfe_planes_configure_extractor")

    def planes_cape_batch(self, depth_m: np.ndarray, K4, patch=20, cos_angle_max=None, max_merge_dist=50.0, cap=64, n_threads=0, seg=False):
        """PlaneDetection_CAPE for a [B, H, W] float32 batch on a pool of host threads -> (planes [B, cap], n [B][, seg [B, H, W]])."""
        d = np.ascontiguousarray(depth_m, np.float32)
        B, h, w = d.shape
        if cos_angle_max is None:
            cos_angle_max = np.float32(np.cos(np.pi / 12))
        planes = np.zeros((B, cap), CAPE_PLANE_DTYPE)
        n = np.zeros(B, np.int32)
        sg = np.zeros((B, h, w), np.uint8) if seg else None
        self._chk(self.L.drfe_planes_cape_batch(self.h, _p(d), w * h, w, h, w, B, _p(np.ascontiguousarray(K4, np.float32)), patch,
                                                np.float32(cos_angle_max), np.float32(max_merge_dist), _p(planes), cap, _p(n), _p(sg),
                                                int(n_threads)), "drfe_planes_cape_batch")
        return (planes, n, sg) if seg else (planes, n)

    def planes_cape(self, depth_m: np.ndarray, K4, patch=20, cos_angle_max=None, max_merge_dist=50.0, cap=64):
        """PlaneDetection_CAPE::readDepthImage + runPlaneDetection -> dict(planes, seg, cell taps)."""
        d = np.ascontiguousarray(depth_m, np.float32)
        h, w = d.shape
        if cos_angle_max is None:
            cos_angle_max = np.float32(np.cos(np.pi / 12))
        nc = (w // patch) * (h // patch)
        planes = np.zeros(cap, CAPE_PLANE_DTYPE)
        n = C.c_int()
        seg = np.zeros((h, w), np.uint8)
        cells = np.zeros((nc, 16))
        mst = np.zeros((nc, 3), np.float32)
        pn = np.zeros((nc, 2), np.int32)
        self._chk(self.L.drfe_planes_cape(self.h, _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)), patch,
                                          np.float32(cos_angle_max), np.float32(max_merge_dist), _p(planes), cap,
                                          C.byref(n), _p(seg), _p(cells), _p(mst), _p(pn)), "drfe_planes_cape")
        return dict(planes=planes[:n.value].copy(), seg=seg, cells=cells, cell_mst=mst, cell_planar=pn[:, 0],
                    cell_npts=pn[:, 1])

    def planes_ahc_blocks(self, depth16: np.ndarray, K4, depth_factor):
        d = np.ascontiguousarray(depth16, np.uint16)
        h, w = d.shape
        nb = (w // 10) * (h // 10)
        blocks = np.zeros((nb, 17))
        vn = np.zeros((nb, 2), np.int32)
        self._chk(self.L.drfe_planes_ahc_blocks(self.h, _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)),
                                                np.float32(depth_factor), _p(blocks), _p(vn), nb), "drfe_planes_ahc_blocks")
        return blocks, vn[:, 0], vn[:, 1]

    # --- plane post-processing + surface normals (Frame::ComputePlanes after the extractor) ------------
    def planes_ahc_postprocess(self, depth16, K4, depth_factor, ahc, max_point_dist, dist_threshold):
        """ahc = the dict planes_ahc returned. -> dict(post, voxels=[per plane [m,3]], n_accepted, plane_num)."""
        d = np.ascontiguousarray(depth16, np.uint16)
        h, w = d.shape
        planes = np.ascontiguousarray(ahc["planes"], PLANE_DTYPE)
        n = len(planes)
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(m) for m in ahc["members"]])
        idx = np.concatenate([np.asarray(m, np.int32) for m in ahc["members"]]) if n else np.zeros(0, np.int32)
        idx = np.ascontiguousarray(idx, np.int32)
        post = np.zeros(n, PLANE_POST_DTYPE)
        vox = np.zeros((max(len(idx), 1), 3), np.float32)
        voff = np.zeros(n + 1, np.int32)
        na, pn = C.c_int(), C.c_int()
        self._chk(self.L.drfe_planes_ahc_postprocess(self.h, _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)),
                                                     np.float32(depth_factor), _p(planes), n, _p(off), _p(idx),
                                                     np.float32(max_point_dist), float(dist_threshold), _p(post), _p(vox),
                                                     _p(voff), len(vox), C.byref(na), C.byref(pn)),
                  "drfe_planes_ahc_postprocess")
        return dict(post=post, voxels=[vox[voff[i]:voff[i + 1]].copy() for i in range(n)], n_accepted=na.value,
                    plane_num=pn.value)

    def planes_ahc_post_batch(self, depth16_batch, K4, depth_factor, max_point_dist, dist_threshold, cap=64, n_threads=0, seg=False):
        """planes_ahc_batch + planes_ahc_postprocess per frame inside the C++ thread pool -> (planes [B,cap], n_planes [B],
        post [B,cap], n_accepted [B], plane_num [B][, seg [B,H,W]])."""
        d = np.ascontiguousarray(depth16_batch, np.uint16)
        B, h, w = d.shape
        planes = np.zeros((B, cap), PLANE_DTYPE)
        post = np.zeros((B, cap), PLANE_POST_DTYPE)
        n, na, pn = (np.zeros(B, np.int32) for _ in range(3))
        sg = np.zeros((B, h, w), np.uint8) if seg else None
        self._chk(self.L.drfe_planes_ahc_post_batch(self.h, _p(d), w * h, w, h, w, B, _p(np.ascontiguousarray(K4, np.float32)),
                                                    np.float32(depth_factor), np.float32(max_point_dist), float(dist_threshold),
                                                    _p(planes), cap, _p(n), _p(sg), _p(post), _p(na), _p(pn), int(n_threads)),
                  "drfe_planes_ahc_post_batch")
        return (planes, n, post, na, pn, sg) if seg else (planes, n, post, na, pn)

    def planes_cape_postprocess(self, depth_m, K4, cape, max_point_dist, dist_threshold):
        """cape = the dict planes_cape returned. -> dict(post, voxels, n_accepted, plane_num)."""
        d = np.ascontiguousarray(depth_m, np.float32)
        h, w = d.shape
        planes = np.ascontiguousarray(cape["planes"], CAPE_PLANE_DTYPE)
        seg = np.ascontiguousarray(cape["seg"], np.uint8)
        n = len(planes)
        post = np.zeros(n, PLANE_POST_DTYPE)
        vox = np.zeros((h * w, 3), np.float32)
        voff = np.zeros(n + 1, np.int32)
        na, pn = C.c_int(), C.c_int()
        self._chk(self.L.drfe_planes_cape_postprocess(self.h, _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)),
                                                      _p(seg), _p(planes), n, np.float32(max_point_dist),
                                                      float(dist_threshold), _p(post), _p(vox), _p(voff), len(vox),
                                                      C.byref(na), C.byref(pn)), "drfe_planes_cape_postprocess")
        return dict(post=post, voxels=[vox[voff[i]:voff[i + 1]].copy() for i in range(n)], n_accepted=na.value,
                    plane_num=pn.value)

    def surface_normals(self, depth_m, K4, max_point_dist, taps=False):
        """vSurfaceNormal of Frame::ComputePlanes for one CV_32F depth image (metres)."""
        d = np.ascontiguousarray(depth_m, np.float32)
        h, w = d.shape
        W, H = (w + 2) // 3, (h + 2) // 3
        out = np.zeros((H // 2) * (W // 2), SURFACE_NORMAL_DTYPE)
        n = C.c_int()
        cloud = np.zeros((H, W, 3), np.float32) if taps else None
        nrm = np.zeros((H, W, 3), np.float32) if taps else None
        dist = np.zeros((H, W), np.float32) if taps else None
        self._chk(self.L.drfe_surface_normals(self.h, _p(d), w, h, w, _p(np.ascontiguousarray(K4, np.float32)),
                                              np.float32(max_point_dist), _p(out), len(out), C.byref(n), _p(cloud), _p(nrm),
                                              _p(dist)), "drfe_surface_normals")
        return (out[:n.value], cloud, nrm, dist) if taps else out[:n.value]

    def surface_normals_batch_ptr(self, d_depth: int, frame_stride: int, row_stride: int, w: int, h: int, K4, depth_factor,
                                  max_point_dist, nframes: int, stream: int = 0):
        self._chk(self.L.drfe_surface_normals_batch(self.h, C.c_void_p(d_depth), frame_stride, row_stride, w, h,
                                                    _p(np.ascontiguousarray(K4, np.float32)), np.float32(depth_factor),
                                                    np.float32(max_point_dist), nframes, C.c_void_p(stream)),
                  "drfe_surface_normals_batch")

    def surface_normals_download(self, slot: int):
        n = C.c_int()
        self._chk(self.L.drfe_surface_normals_download(self.h, slot, None, 0, C.byref(n)), "drfe_surface_normals_download")
        out = np.zeros(n.value, SURFACE_NORMAL_DTYPE)
        self._chk(self.L.drfe_surface_normals_download(self.h, slot, _p(out), len(out), C.byref(n)),
                  "drfe_surface_normals_download")
        return out

    def manhattan_track_batch(self, R0, nseq: int, seq_len: int, line_dirs=None, line_offsets=None, n_calls=3, stream: int = 0):
        """Manhattan-frame tracking of nseq sequences of seq_len frames of the most recent surface_normals_batch_ptr (frame
        s * seq_len + t = frame t of sequence s); R0: nseq x 3 x 3 starting rotations; line_dirs (n x 3 float64) with
        line_offsets (nseq * seq_len + 1) or None."""
        R0 = np.ascontiguousarray(R0, np.float32).reshape(nseq, 9)
        if line_dirs is not None:
            line_dirs = np.ascontiguousarray(line_dirs, np.float64).reshape(-1, 3)
            line_offsets = np.ascontiguousarray(line_offsets, np.int32)
            if len(line_offsets) != nseq * seq_len + 1 or line_offsets[-1] != len(line_dirs):
                raise ValueError("line_offsets must have nseq * seq_len + 1 entries ending at len(line_dirs)")
        self._frame_lines = None if line_offsets is None else line_offsets.copy()
        self._chk(self.L.drfe_manhattan_track_batch(self.h, _p(R0), nseq, seq_len, _p(line_dirs), _p(line_offsets), n_calls,
                                                    C.c_void_p(stream)), "drfe_manhattan_track_batch")

    def manhattan_download(self, frame: int, n_records: int):
        """(R 3x3 float32, info, rec_bits uint16[n_records], line_bits uint16) of one frame of the most recent batch"""
        lo = getattr(self, "_frame_lines", None)
        nl = 0 if lo is None else int(lo[frame + 1] - lo[frame])
        R = np.zeros((3, 3), np.float32)
        info = np.zeros((), MANHATTAN_INFO_DTYPE)
        rb = np.zeros(n_records, np.uint16)
        lb = np.zeros(nl, np.uint16)
        self._chk(self.L.drfe_manhattan_download(self.h, frame, _p(R), _p(info), _p(rb), _p(lb) if nl else None),
                  "drfe_manhattan_download")
        return R, info, rb, lb

    # --- plane association (PlaneMatcher / Map::FlagMatchedPlanePoints) over device-resident maps --------
    def plane_map_upload(self, maps):
        """maps: list of dict(coefs [M, 4] world, bad [M], clouds (list of M [n, 3]), points [N, 3]) -> drfe_plane_map_upload"""
        poff = np.zeros(len(maps) + 1, np.int32)
        poff[1:] = np.cumsum([len(m["coefs"]) for m in maps])
        qoff = np.zeros(len(maps) + 1, np.int32)
        qoff[1:] = np.cumsum([len(m["points"]) for m in maps])
        coefs = np.ascontiguousarray(np.concatenate([np.asarray(m["coefs"], np.float32).reshape(-1, 4) for m in maps]), np.float32)
        bad = np.ascontiguousarray(np.concatenate([np.asarray(m["bad"], np.uint8).reshape(-1) for m in maps]), np.uint8)
        coff, cloud = _clouds_csr([c for m in maps for c in m["clouds"]])
        pts = np.ascontiguousarray(np.concatenate([np.asarray(m["points"], np.float32).reshape(-1, 3) for m in maps]), np.float32)
        self._plane_points = [len(m["points"]) for m in maps]
        self._chk(self.L.drfe_plane_map_upload(self.h, len(maps), _p(poff), _p(coefs), _p(bad), _p(coff), _p(cloud), _p(qoff),
                                               _p(pts)), "drfe_plane_map_upload")

    def plane_match_batch(self, frame_map, Tcw, coefs, map_idx=None, par_idx=None, ver_idx=None, flag_points=True, params=None,
                          stream: int = 0):
        """frame f (Tcw [F, 4, 4], coefs[f] [P_f, 4]) against uploaded map frame_map[f]; priors: per-frame lists of index
        arrays or None"""
        F = len(frame_map)
        fm = np.ascontiguousarray(frame_map, np.int32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(F, 16)
        off = np.zeros(F + 1, np.int32)
        off[1:] = np.cumsum([len(np.asarray(c).reshape(-1, 4)) for c in coefs])
        cf = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float32).reshape(-1, 4) for c in coefs]), np.float32)
        pri = [None if p is None else np.ascontiguousarray(np.concatenate([_priors(p[f], off[f + 1] - off[f]) for f in range(F)]),
                                                            np.int32) for p in (map_idx, par_idx, ver_idx)]
        prm = _plane_params(params)
        self._plane_frames = off.copy()
        self._chk(self.L.drfe_plane_match_batch(self.h, _p(prm), F, _p(fm), _p(T), _p(off), _p(cf), _p(pri[0]), _p(pri[1]),
                                                _p(pri[2]), int(bool(flag_points)), C.c_void_p(stream)), "drfe_plane_match_batch")

    def plane_match_download(self, frame: int):
        """(map_idx, par_idx, ver_idx, nmatches, n_pairs) of one frame of the most recent plane_match_batch"""
        P = int(self._plane_frames[frame + 1] - self._plane_frames[frame])
        mi, pi, vi = (np.zeros(P, np.int32) for _ in range(3))
        nm, npair = C.c_int(), C.c_int()
        self._chk(self.L.drfe_plane_match_download(self.h, frame, _p(mi), _p(pi), _p(vi), C.byref(nm), C.byref(npair)),
                  "drfe_plane_match_download")
        return mi, pi, vi, nm.value, npair.value

    def plane_flags_download(self, map_id: int):
        """uint8 flags of the map's points: the OR over the frames of that map in the most recent batch"""
        out = np.zeros(max(self._plane_points[map_id], 1), np.uint8)
        self._chk(self.L.drfe_plane_flags_download(self.h, map_id, _p(out)), "drfe_plane_flags_download")
        return out[:self._plane_points[map_id]]

    def plane_map_update_batch(self, frame_map, Tcw, clouds, map_idx=None, stream: int = 0):
        """MapPlane::UpdateCoefficientsAndPoints(F, i) on the resident maps: frame f (Tcw [F, 4, 4], clouds[f] = list of its
        planes' voxel clouds [n, 3]) updates the planes of map frame_map[f] named by map_idx[f] (plane-local, -1 = none);
        map_idx None = the decisions of the most recent plane_match_batch over the same frames."""
        F = len(frame_map)
        fm = np.ascontiguousarray(frame_map, np.int32)
        T = np.ascontiguousarray(Tcw, np.float32).reshape(F, 16)
        off = np.zeros(F + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in clouds])
        coff, xyz = _clouds_csr([p for c in clouds for p in c])
        mi = None if map_idx is None else np.ascontiguousarray(
            np.concatenate([_priors(map_idx[f], off[f + 1] - off[f]) for f in range(F)]) if off[-1] else np.zeros(0), np.int32)
        self._chk(self.L.drfe_plane_map_update_batch(self.h, F, _p(fm), _p(T), _p(off), _p(coff), _p(xyz), _p(mi), C.c_void_p(stream)),
                  "drfe_plane_map_update_batch")

    def plane_map_rebuild_batch(self, jobs, stream: int = 0):
        """MapPlane::UpdateCoefficientsAndPoints() on the resident maps: jobs = list of (map, plane, observations), each
        observation a (Twc 4x4, cloud [n, 3]) pair in the order the caller iterates them"""
        jm = np.ascontiguousarray([j[0] for j in jobs], np.int32)
        jp = np.ascontiguousarray([j[1] for j in jobs], np.int32)
        ooff = np.zeros(len(jobs) + 1, np.int32)
        ooff[1:] = np.cumsum([len(j[2]) for j in jobs])
        obs = [o for j in jobs for o in j[2]]
        T = np.ascontiguousarray(np.asarray([o[0] for o in obs], np.float32).reshape(-1, 16), np.float32)
        coff, xyz = _clouds_csr([o[1] for o in obs])
        self._chk(self.L.drfe_plane_map_rebuild_batch(self.h, len(jobs), _p(jm), _p(jp), _p(ooff), _p(T), _p(coff), _p(xyz),
                                                      C.c_void_p(stream)), "drfe_plane_map_rebuild_batch")

    def plane_map_edit(self, map_id: int, plane_index, coefs=None, bad=None):
        """SetWorldPos / SetBadFlag of existing planes; an index equal to the plane count appends a plane with an empty cloud"""
        pi = np.ascontiguousarray(plane_index, np.int32).reshape(-1)
        cf = None if coefs is None else np.ascontiguousarray(coefs, np.float32).reshape(len(pi), 4)
        bd = None if bad is None else np.ascontiguousarray(bad, np.uint8).reshape(len(pi))
        self._chk(self.L.drfe_plane_map_edit(self.h, map_id, len(pi), _p(pi), _p(cf), _p(bd)), "drfe_plane_map_edit")

    def plane_map_cloud_download(self, map_id: int, plane: int):
        """the current cloud [n, 3] of one resident map plane"""
        n = C.c_int()
        self._chk(self.L.drfe_plane_map_cloud_download(self.h, map_id, plane, None, 0, C.byref(n)), "drfe_plane_map_cloud_download")
        out = np.zeros((max(n.value, 1), 3), np.float32)
        self._chk(self.L.drfe_plane_map_cloud_download(self.h, map_id, plane, _p(out), n.value, C.byref(n)),
                  "drfe_plane_map_cloud_download")
        return out[:n.value].copy()

    def plane_map_update_stats(self):
        """dict(device_jobs, host_jobs, rounds, repacks) since plane_map_upload"""
        st = np.zeros(4, np.int64)
        self._chk(self.L.drfe_plane_map_update_stats(self.h, _p(st)), "drfe_plane_map_update_stats")
        return dict(zip(("device_jobs", "host_jobs", "rounds", "repacks"), st.tolist()))

    def plane_map_cull_batch(self, map_id: int, scene, mode: int = PLANE_CULL_DISPATCH, rebuilt_capacity=None, stream: int = 0):
        """LocalMapping::MapPlaneCulling on resident map map_id (drfe_plane_map_cull_batch): scene as plane_map_cull_host takes it,
        its coefs / bad / clouds unread (they are resident).  Same result dict; the bad flags and the rebuilt clouds are
        committed into the resident map."""
        cin, cout, keep, o = _plane_cull_pack(scene, rebuilt_capacity)
        self._chk(self.L.drfe_plane_map_cull_batch(self.h, map_id, C.byref(cin), int(mode), C.byref(cout), C.c_void_p(stream)),
                  "drfe_plane_map_cull_batch")
        return _plane_cull_result(cin, cout, o)

    def plane_map_cull_limits(self):
        return plane_map_cull_limits()

    def plane_map_cull_stats(self):
        """dict(calls, device_calls, dist_launches, rebuild_calls) since plane_map_upload"""
        st = np.zeros(4, np.int64)
        self._chk(self.L.drfe_plane_map_cull_stats(self.h, _p(st)), "drfe_plane_map_cull_stats")
        return dict(zip(PLANE_CULL_STATS, st.tolist()))

    def map_point_upkeep_batch(self, scene, what=3, frustum=True):
        """map_point_upkeep_host on the device (drfe_map_point_upkeep_batch): same outputs, same bits"""
        rc, r = _upkeep_call(self.L.drfe_map_point_upkeep_batch, (self.h,), False, scene, what, frustum)
        self._chk(rc, "drfe_map_point_upkeep_batch")
        return r

    def map_line_upkeep_batch(self, scene, what=3, frustum=True):
        """map_line_upkeep_host on the device (drfe_map_line_upkeep_batch)"""
        rc, r = _upkeep_call(self.L.drfe_map_line_upkeep_batch, (self.h,), True, scene, what, frustum)
        self._chk(rc, "drfe_map_line_upkeep_batch")
        return r

    def map_upkeep_stats(self):
        """dict(calls, items, desc_b4, desc_b16, desc_b64, desc_wg, desc_host, normals) since the context was created"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_map_upkeep_stats(self.h, _p(st)), "drfe_map_upkeep_stats")
        return dict(zip(UPKEEP_STATS, st.tolist()))

    def triangulate_points_batch(self, scene, monocular=0):
        """triangulate_points_host on the device (drfe_triangulate_points_batch): same outputs, same bits"""
        rc, r = _tri_call(self.L.drfe_triangulate_points_batch, (self.h,), False, scene, monocular)
        self._chk(rc, "drfe_triangulate_points_batch")
        return r

    def triangulate_lines_batch(self, scene, monocular=0):
        """triangulate_lines_host on the device (drfe_triangulate_lines_batch)"""
        rc, r = _tri_call(self.L.drfe_triangulate_lines_batch, (self.h,), True, scene, monocular)
        self._chk(rc, "drfe_triangulate_lines_batch")
        return r

    def triangulate_math(self, which, y, x=None):
        """triangulate_math on the device (drfe_debug_triangulate_math_device, a kernel of triangulate_kernels.hip): same bits"""
        y = np.ascontiguousarray(y, np.float32)
        x = np.ascontiguousarray(np.zeros_like(y) if x is None else x, np.float32)
        out = np.zeros_like(y)
        self._chk(self.L.drfe_debug_triangulate_math_device(self.h, which, _p(y), _p(x), len(y), _p(out)),
                  "drfe_debug_triangulate_math_device")
        return out

    def triangulate_stats(self):
        """dict(calls, pairs, pairs_skipped, matches, svd, stereo1, stereo2, accepted) since the context was created"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_triangulate_stats(self.h, _p(st)), "drfe_triangulate_stats")
        return dict(zip(TRI_STATS, st.tolist()))

    def sim3_ransac_batch(self, problems):
        """sim3_ransac_host on the device (drfe_sim3_ransac_batch): same table, same bits"""
        rc, r = _sim3_call(self.L.drfe_sim3_ransac_batch, (self.h,), problems)
        self._chk(rc, "drfe_sim3_ransac_batch")
        return r

    def pnp_ransac_batch(self, problems):
        """pnp_ransac_host on the device (drfe_pnp_ransac_batch): same table, same bits"""
        rc, r = _pnp_call(self.L.drfe_pnp_ransac_batch, (self.h,), problems)
        self._chk(rc, "drfe_pnp_ransac_batch")
        return r

    def pose_opt_batch(self, problems):
        """pose_opt_host on the device (drfe_pose_opt_batch): same outputs, same bits"""
        P, out, r, _keep = _pose_opt_pack(problems)
        self._chk(self.L.drfe_pose_opt_batch(self.h, C.byref(P), C.byref(out), None), "drfe_pose_opt_batch")
        return r

    def pose_opt_stats(self):
        """drfe_pose_opt_stats as a dict over POSE_OPT_STATS"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_pose_opt_stats(self.h, _p(st)), "drfe_pose_opt_stats")
        return dict(zip(POSE_OPT_STATS, st.tolist()))

    def pose_opt_hand_back(self, every):
        """test hook: the host runs every `every`-th frame of a batch call again as if the device had not certified it"""
        self._chk(self.L.drfe_debug_pose_opt_hand_back(self.h, int(every)), "drfe_debug_pose_opt_hand_back")

    def trans_opt_batch(self, problems):
        """trans_opt_host on the device (drfe_trans_opt_batch): same outputs, same bits"""
        P, out, r, _keep = _pose_opt_pack(problems)
        self._chk(self.L.drfe_trans_opt_batch(self.h, C.byref(P), C.byref(out), None), "drfe_trans_opt_batch")
        return r

    def trans_opt_stats(self):
        """drfe_trans_opt_stats as a dict over POSE_OPT_STATS"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_trans_opt_stats(self.h, _p(st)), "drfe_trans_opt_stats")
        return dict(zip(POSE_OPT_STATS, st.tolist()))

    def trans_opt_hand_back(self, every):
        """test hook: the host runs every `every`-th frame of a trans_opt_batch call again as if the device had handed it back"""
        self._chk(self.L.drfe_debug_trans_opt_hand_back(self.h, int(every)), "drfe_debug_trans_opt_hand_back")

    def sim3_opt_batch(self, problems):
        """sim3_opt_host on the device (drfe_sim3_opt_batch): same outputs, same bits"""
        P, out, r, _keep = _sim3_opt_pack(problems)
        self._chk(self.L.drfe_sim3_opt_batch(self.h, C.byref(P), C.byref(out), None), "drfe_sim3_opt_batch")
        return r

    def sim3_opt_stats(self):
        """drfe_sim3_opt_stats as a dict over SIM3_OPT_STATS"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_sim3_opt_stats(self.h, _p(st)), "drfe_sim3_opt_stats")
        return dict(zip(SIM3_OPT_STATS, st.tolist()))

    def sim3_opt_hand_back(self, every):
        """test hook: the host runs every `every`-th problem of a sim3_opt_batch call again as if the device had not certified it"""
        self._chk(self.L.drfe_debug_sim3_opt_hand_back(self.h, int(every)), "drfe_debug_sim3_opt_hand_back")

    def init_ransac_batch(self, problems):
        """init_ransac_host on the device (drfe_init_ransac_batch): same outputs, same bits"""
        rc, r = _init_call(self.L.drfe_init_ransac_batch, (self.h,), problems)
        self._chk(rc, "drfe_init_ransac_batch")
        return r

    def init_stats(self):
        """drfe_init_stats as a dict over INIT_STATS"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_init_stats(self.h, _p(st)), "drfe_init_stats")
        return dict(zip(INIT_STATS, (int(v) for v in st)))

    def pnp_stats(self):
        """dict(calls, solvers, hypotheses, correspondences, refine_jobs, refine_points, solvers_global, solvers_empty) since the
        context was created; solvers - solvers_empty - solvers_global were counted from LDS"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_pnp_stats(self.h, _p(st)), "drfe_pnp_stats")
        return dict(zip(PNP_STATS, st.tolist()))

    def lines_is_good_batch(self, lines, n_lines, depth, K9, cx, cy, invfx, invfy, k_as_f64=True, seeds=None, w=None):
        """lines_is_good for the key lines of F frames in one device call (drfe_lines_is_good_batch, arguments as line3d_frames):
        (depth_line [F, cap], lines3d [F, cap, 6], n_inliers [F, cap], n_good [F]); frame f's first n_lines[f] entries are, byte for
        byte, what lines_is_good gives with seed = seeds[f] (default 1), the others -1 / 0"""
        fr, out, r, _keep = line3d_frames(lines, n_lines, depth, K9, cx, cy, invfx, invfy, k_as_f64, seeds, w)
        self._chk(self.L.drfe_lines_is_good_batch(self.h, C.byref(fr), C.byref(out), None), "drfe_lines_is_good_batch")
        return r

    def line3d_stats(self):
        """dict(calls, frames, lines, ransac_lines, iterations, coincident_pairs, verify_rejections, accepted) since the context
        was created"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_line3d_stats(self.h, _p(st)), "drfe_line3d_stats")
        return dict(zip(LINE3D_STATS, st.tolist()))

    def sim3_hand_back(self, every):
        """test hook: the host finishes every `every`-th hypothesis of a batch call as if the device had not certified it"""
        self._chk(self.L.drfe_debug_sim3_hand_back(self.h, int(every)), "drfe_debug_sim3_hand_back")

    def sim3_stats(self):
        """dict(calls, solvers, hypotheses, correspondences, solvers_lds, solvers_global, uncertified, solvers_empty) since the
        context was created"""
        st = np.zeros(8, np.int64)
        self._chk(self.L.drfe_sim3_stats(self.h, _p(st)), "drfe_sim3_stats")
        return dict(zip(SIM3_STATS, st.tolist()))

    # --- measurement -------------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._chk(self.L.drfe_profile_enable(self.h, int(on)), "drfe_profile_enable")

    def profile_stage_ms(self):
        ms = np.zeros(len(STAGES), np.float32)
        self._chk(self.L.drfe_profile_stage_ms(self.h, _p(ms)), "drfe_profile_stage_ms")
        return dict(zip(STAGES, ms.tolist()))

    def sync(self):
        self._chk(self.L.drfe_stream_sync(self.h), "drfe_stream_sync")
