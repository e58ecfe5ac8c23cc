"""ctypes binding of the C-ABI in include/misift.h (libmisift.so).

Thin by design: every method is one C call plus argument marshalling.  There is NO
CPU fallback — if the HIP library is missing or fails to load, importing the
binding's `lib()` raises, and every GPU entry point fails loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MISIFT_LIB: developer override to A/B-test another build of the same library (tools/variants.sh)
LIB_PATH = os.environ.get("MISIFT_LIB") or os.path.join(HERE, "libmisift.so")

POINT_DTYPE = np.dtype([
    ("xpos", "<f4"), ("ypos", "<f4"), ("scale", "<f4"), ("sharpness", "<f4"),
    ("edgeness", "<f4"), ("orientation", "<f4"), ("score", "<f4"), ("ambiguity", "<f4"),
    ("match", "<i4"), ("match_xpos", "<f4"), ("match_ypos", "<f4"), ("match_error", "<f4"),
    ("subsampling", "<f4"), ("empty", "<f4", (3,)), ("data", "<f4", (128,)),
])
assert POINT_DTYPE.itemsize == 576


# misift_track_obs: one observation of an exported track (misift_export_tracks_batch)
TRACK_OBS_DTYPE = np.dtype([("frame", "<i4"), ("record", "<i4"), ("xpos", "<f4"), ("ypos", "<f4")])
CAM_UNSET, CAM_ROOT, CAM_RESECTED, CAM_MERGED = -2, -1, -3, -4  # cam_pair values that are no pair index
# the arguments that state one scene to merge_scenes_batch, in the order of the C call; the last two are optional
MERGE_SCENE_KEYS = ("max_tracks", "max_obs", "track_offsets", "obs", "export_summary", "points", "point_views",
                    "point_status", "nimages", "cam", "cam_pair", "max_records", "record_obs")
MERGE_OUTPUTS = ("track_offsets_out", "obs_out", "export_summary_out", "points_out", "point_views_out",
                 "point_status_out", "cam_out", "cam_pair_out", "track_map_a", "obs_map_a", "obs_map_b",
                 "record_obs_out", "summary")
LOSS_NONE, LOSS_HUBER, LOSS_GEMAN_MCCLURE = 0, 1, 2            # MISIFT_LOSS_*: adjust_bundle_robust_batch
MAX_FOCAL_GROUPS = 8                                           # MISIFT_MAX_FOCAL_GROUPS: adjust_bundle_focal_batch
FOCAL_REFINED, FOCAL_NO_MEMBER, FOCAL_NOT_REFINED = 0, 1, 2    # MISIFT_FOCAL_*: d_focal[3g + 2]
MAX_RADIAL_GROUPS = MAX_FOCAL_GROUPS                           # MISIFT_MAX_RADIAL_GROUPS: adjust_bundle_radial_batch
RADIAL_REFINED, RADIAL_NO_MEMBER, RADIAL_NOT_REFINED, RADIAL_HELD = 0, 1, 2, 3   # MISIFT_RADIAL_*: d_radial[3g + 2]
assert TRACK_OBS_DTYPE.itemsize == 16


class Options(C.Structure):
    _fields_ = [("texfrac_bits", C.c_int), ("fix_numpts", C.c_int), ("match_full", C.c_int),
                ("match_exact_top2", C.c_int), ("quiet", C.c_int), ("fused", C.c_int), ("deterministic", C.c_int),
                ("reference_cap", C.c_int)]


class MisiftError(RuntimeError):
    pass


# name -> (restype, argtypes); also the list the symbol-export test checks against the header
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_ip, _fp, _up = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint)
SIGNATURES = {
    "misift_device_count": (_i, []),
    "misift_device_info": (_i, [_i, C.c_char_p, _i, _ip, _ip, C.POINTER(_sz), _ip, _ip]),
    "misift_device_arch": (_i, [_i, C.c_char_p, _i]),
    "misift_ctx_create": (_i, [_i, _vp, C.POINTER(_vp)]),
    "misift_ctx_destroy": (None, [_vp]),
    "misift_ctx_set_stream": (_i, [_vp, _vp]),
    "misift_ctx_set_graph_replay": (_i, [_vp, _i]),
    "misift_ctx_sync": (_i, [_vp]),
    "misift_ctx_set_early_return": (_i, [_vp, _i]),
    "misift_ctx_chain_fallbacks": (_i, [_vp]),
    "misift_ctx_fuse_fallbacks": (_i, [_vp]),
    "misift_ctx_last_call_balanced": (_i, [_vp]),
    "misift_ctx_descr_big_fallbacks": (_i, [_vp]),
    "misift_last_error": (C.c_char_p, []),
    "misift_default_options": (None, [C.POINTER(Options)]),
    "misift_default_options_sized": (None, [C.POINTER(Options), C.c_size_t]),
    "misift_set_options": (_i, [_vp, C.POINTER(Options)]),
    "misift_get_options": (_i, [_vp, C.POINTER(Options)]),
    "misift_set_options_sized": (_i, [_vp, C.POINTER(Options), C.c_size_t]),
    "misift_get_options_sized": (_i, [_vp, C.POINTER(Options), C.c_size_t]),
    "misift_malloc": (_i, [_sz, C.POINTER(_vp)]),
    "misift_free": (_i, [_vp]),
    "misift_memset": (_i, [_vp, _vp, _i, _sz]),
    "misift_copy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "misift_copy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "misift_image_alloc": (_i, [_i, _i, C.POINTER(_vp), _ip]),
    "misift_upload_2d": (_i, [_vp, _vp, _i, _vp, _i, _i, _i]),
    "misift_download_2d": (_i, [_vp, _vp, _i, _vp, _i, _i, _i]),
    "misift_download_fields": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "misift_scratch_floats": (_sz, [_i, _i, _i, _i]),
    "misift_extract": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _f, _f, _i, _vp, _vp, _i, _ip]),
    "misift_extract_batch": (_i, [_vp, _vp, _i, _sz, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _ip]),
    "misift_extract_batch_async": (_i, [_vp, _vp, _i, _sz, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _vp]),
    "misift_get_counters": (_i, [_vp, _i, _up]),
    "misift_get_counter_block": (_i, [_vp, _i, _up]),
    "misift_set_counters": (_i, [_vp, _i, _up]),
    "misift_lowpass": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _f]),
    "misift_scaledown": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "misift_scaleup": (_i, [_vp, _vp, _i, _i, _i, _vp, _i]),
    "misift_laplace_taps": (_i, [_i, _fp]),
    "misift_laplace": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "misift_reset_counters": (_i, [_vp, _i]),
    "misift_findpoints": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _f, _f, _i, _vp, _i]),
    "misift_dog_findpoints": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _f, _vp, _i]),
    "misift_orientations": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i]),
    "misift_descriptors": (_i, [_vp, _vp, _i, _i, _i, _f, _i, _vp, _i]),
    "misift_rescale_positions": (_i, [_vp, _vp, _i, _f]),
    "misift_match": (_i, [_vp, _vp, _i, _vp, _i]),
    "misift_match_rows": (_i, [_vp, _vp, _i, _i, _vp, _i]),
    "misift_improve_homography": (_i, [_vp, _vp, _i, _fp, _i, _f, _f, _f, _ip]),
    "misift_malloc_managed": (_i, [_sz, C.POINTER(_vp)]),
    "misift_ctx_set_batches_in_flight": (_i, [_vp, _i]),
    "misift_ctx_get_batches_in_flight": (_i, [_vp]),
    "misift_ctx_wait_batch": (_i, [_vp, _vp]),
    "misift_ctx_record_batch": (_i, [_vp, _vp]),
    "misift_test_elementary": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i]),
    "misift_test_match_split": (_i, [_vp, _vp, _i, _vp, _i, _i, _i]),
    "misift_test_match_plan": (_i, [_i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "misift_test_match_batch_plan": (_i, [_i, _i, _i, _vp, _vp, _vp, _ip, _ip, _ip]),
    "misift_match_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i]),
    "misift_match_pairs_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp,
                                      _vp]),
    "misift_find_homography_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _vp]),
    "misift_improve_homography_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp]),
    "misift_find_fundamental_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _f, _f, _f, _vp, _vp]),
    "misift_score_fundamental_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _f, _f, _f, _vp, _vp]),
    "misift_improve_fundamental_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp]),
    "misift_recover_pose_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp, _vp, _vp]),
    "misift_recover_pose_planar_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _f, _f, _f, _f, _f, _i, _f, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_link_poses_batch": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _f, _f, _f, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i,
                                     _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_match_guided_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _f, _i, _vp]),
    "misift_match_epipolar_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _f, _i, _vp]),
    "misift_quantize_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp]),
    "misift_match_batch_i8": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i]),
    "misift_match_pairs_batch_i8": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i,
                                         _vp, _vp, _vp]),
    "misift_link_tracks_batch": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _f, _f, _f, _vp, _vp, _vp, _vp]),
    "misift_export_tracks_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp,
                                        _vp]),
    "misift_triangulate_tracks_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                             _vp]),
    "misift_test_triangulate_track": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_triangulate_capacity": (_i, []),
    "misift_refine_cameras_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _f, _i,
                                         _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_refine_camera": (_i, [_vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp]),
    "misift_adjust_bundle_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i,
                                        _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_adjust_bundle_robust_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i,
                                               _i, _f, _f, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_adjust_bundle_robust": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i,
                                              _f, _f, _i, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_adjust_bundle_focal_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i,
                                              _i, _f, _f, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp]),
    "misift_test_adjust_bundle_focal": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i,
                                             _f, _f, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                             _vp, _vp]),
    "misift_adjust_bundle_radial_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i,
                                               _i, _f, _f, _i, _i, _f, _i, _vp, _vp, _vp] + 13 * [_vp]),
    "misift_test_adjust_bundle_radial": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i,
                                              _f, _f, _i, _i, _f, _i, _vp, _vp, _vp] + 13 * [_vp]),
    "misift_undistort_obs_batch": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "misift_test_undistort_obs": (_i, [_i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    "misift_test_adjust_bundle": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _f, _f,
                                       _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_filter_tracks_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_filter_tracks": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_filter_stage": (_i, []),
    "misift_resect_cameras_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _f, _i, _i,
                                         _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_resect_samples": (_i, [C.c_uint, _i, _i, _vp]),
    "misift_test_resect_solve": (_i, [_vp, _vp, _vp, _vp]),
    "misift_describe_points_batch": (_i, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp,
                                          _vp, _vp]),
    "misift_test_describe_points": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                         _vp]),
    "misift_localize_frames_batch": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _i,
                                          _f, _f, _i, _f, _i, _i, _i] + 7 * [_vp] + [_i] + 7 * [_vp]),
    "misift_test_localize_candidates": (_i, [_vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp]),
    "misift_correspond_tracks_batch": (_i, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "misift_align_points_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _f, _i, _i, _vp, _vp, _vp,
                                       _vp, _vp, _vp]),
    "misift_transform_scene_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "misift_merge_scenes_batch": (_i, [_vp] + 2 * [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp] +
                                  [_vp, _vp] + 8 * [_i] + 13 * [_vp]),
    "misift_test_merge_scenes": (_i, 2 * [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp] + [_vp, _vp] +
                                 8 * [_i] + 13 * [_vp]),
    "misift_test_merge_capacity": (_i, []),
    "misift_test_align_samples": (_i, [C.c_uint, _i, _i, _vp]),
    "misift_test_align_solve": (_i, [_vp, _vp, _vp, _vp]),
    "misift_test_align_refit": (_i, [_vp, _vp, _i, _f, _i, _vp, _vp, _vp]),
    "misift_test_transform_camera": (_i, [_vp, _vp, _vp]),
    "misift_test_transform_point": (_i, [_vp, _vp, _vp]),
    "misift_select_pairs_batch": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp,
                                       _vp]),
    "misift_test_select_pairs": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _f, _f, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_quantize": (_i, [_vp, C.c_long, _vp]),
    "misift_test_match_i8_plan": (_i, [_i, _i, _vp, _vp, _vp, _ip, _ip, _ip]),
    "misift_test_libc_rand": (_i, [C.c_uint, _i, _vp]),
    "misift_test_homography_samples": (_i, [C.c_uint, _i, _i, _vp]),
    "misift_test_fundamental_samples": (_i, [C.c_uint, _i, _i, _vp]),
    "misift_test_fundamental_solve": (_i, [_vp, _vp, _vp]),
    "misift_test_fundamental_sampson": (_i, [_vp, _vp, _i, _vp, _vp]),
    "misift_test_fundamental_error": (_i, [_vp, _vp, _i, _vp]),
    "misift_test_fundamental_refine": (_i, [_vp, _vp, _i, _vp, _f, _i, _vp, _vp, _vp]),
    "misift_test_fundamental_refine_capacity": (_i, []),
    "misift_test_fundamental_solve9": (_i, [_vp, _i, _vp, _vp]),
    "misift_test_pose_decompose": (_i, [_vp, _vp, _vp, _vp]),
    "misift_test_pose_vote": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "misift_test_pose_planar_decompose": (_i, [_vp, _vp, _f, _vp, _vp]),
    "misift_test_pose_planar_vote": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "misift_test_posegraph_ratio": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _f, _f, _f, _i, _vp, _vp]),
    "misift_test_posegraph_compose": (_i, [_i, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_posegraph_capacity": (_i, [_i]),
    "misift_test_epipolar_gate": (_i, [_vp, _vp, _i, _vp, _i, _f, _vp]),
    "misift_test_epipolar_gather": (_i, [_vp, _vp, _i, _vp, _i, _f, _vp, _vp]),
    "misift_test_guided_gather": (_i, [_vp, _vp, _i, _vp, _i, _f, _vp, _vp, _vp]),
    "misift_test_frame_shares": (_i, [_i, _i, C.c_void_p, C.c_void_p]),
    "misift_test_block_maps": (_i, [_vp, _ip, _ip, _vp, _i]),
    "misift_test_strip_geom": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "misift_test_pyramid_layout": (_i, [_i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "misift_test_describe_detections": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp]),
    "misift_test_detect_levels": (_i, [_vp, _i, _i, _i, _i, _f, _f, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "misift_test_set_knob": (_i, [_vp, C.c_char_p, C.c_double]),
    "misift_test_knob_names": (C.c_char_p, []),
    "misift_test_set_guard": (_i, [_i]),
    "misift_test_check_guards": (_i, [C.POINTER(_i)]),
    "misift_test_ctx_state": (C.c_longlong, [_vp, _i]),
    "misift_comm_unique_id": (_i, [_vp]),
    "misift_comm_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "misift_comm_adopt": (_i, [_vp, _vp, C.POINTER(_vp)]),
    "misift_loopback_world_create": (_i, [_i, C.POINTER(_vp)]),
    "misift_loopback_world_destroy": (None, [_vp]),
    "misift_comm_create_loopback": (_i, [_vp, _vp, _i, C.POINTER(_vp)]),
    "misift_gather_test": (_i, [_vp, _i, _ip]),
    "misift_comm_destroy": (None, [_vp]),
    "misift_comm_rank": (_i, [_vp]),
    "misift_comm_size": (_i, [_vp]),
    "misift_comm_barrier": (_i, [_vp]),
    "misift_gather_post": (_i, [_vp, _vp, _i, _vp, _i, _vp]),
    "misift_gather_complete": (_i, [_vp, _i, _i, _vp, _vp, _sz, _vp]),
    "misift_match_sharded": (_i, [_vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "misift_comm_wire_bytes": (_i, [_vp, _vp, _vp]),
    "misift_comm_create_host": (_i, [_i, _i, _vp, _vp]),
    "misift_find_homography": (_i, [_vp, _vp, _i, _fp, _ip, _i, _f, _f, _f]),
    "misift_extract_batch_packed_async": (_i, [_vp, _vp, _i, _sz, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _vp, _vp, _vp]),
    "misift_lowpass_scaledown": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _f, _vp, _i]),
    "misift_extract_batch_u8": (_i, [_vp, _vp, _i, _sz, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _i, _ip]),
    "misift_extract_batch_ex": (_i, [_vp, _vp, _i, _i, _sz, _i, _i, _i, _i, _f, _f, _f, _i, _vp, _vp, _i, _ip]),
    "misift_pipe_create": (_i, [_vp, _i, _i, _i, _i, _i, _f, _f, _f, _i, _i, C.POINTER(_vp)]),
    "misift_pipe_destroy": (None, [_vp]),
    "misift_pipe_submit": (_i, [_vp, _vp, _i]),
    "misift_pipe_collect": (_i, [_vp, _ip, _ip, _vp, _sz, C.POINTER(_sz)]),
    "misift_pipe_pending": (_i, [_vp]),
    "misift_host_alloc": (_i, [_sz, C.POINTER(_vp)]),
    "misift_host_free": (_i, [_vp]),
    "misift_timer_start": (_i, [_vp]),
    "misift_timer_stop_ms": (_i, [_vp, _fp]),
    "misift_profile_enable": (_i, [_vp, _i]),
    "misift_profile_reset": (_i, [_vp]),
    "misift_profile_read": (_i, [_vp, _i, _vp, _fp, _ip, _ip]),
}

_lib = None


def lib():
    """Load libmisift.so (raises if it is missing: the HIP path is the only path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MisiftError("HIP extension %s is not built — run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` or `make`" % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def hip_runtime():
    """The HIP runtime libmisift.so is bound to, as a ctypes handle of its own (symbols are looked up through libmisift's
    dependencies): where raw streams and events that are handed to the library come from.  C.CDLL("libamdhip64.so") can
    be another runtime: torch bundles one and loads it under that name when it is imported after libmisift, and a stream
    or event of the one aborts inside the other."""
    lib()
    return C.CDLL(LIB_PATH)


def check(rc, what=""):
    if rc != 0:
        raise MisiftError("%s failed (rc=%d): %s" % (what, rc, lib().misift_last_error().decode()))


def device_count():
    return lib().misift_device_count()


def scratch_floats(width, height, num_octaves=5, scale_up=False):
    return int(lib().misift_scratch_floats(width, height, num_octaves, int(scale_up)))


def pyramid_layout(width, height, num_octaves=5, scale_up=False):
    """misift_test_pyramid_layout (host-only): [(float offset inside one frame's arena, w, h, pitch)] of the pyramid levels
    num_octaves ... 1, finest first."""
    off = np.zeros(num_octaves, np.int64)
    w, h, p = (np.zeros(num_octaves, np.int32) for _ in range(3))
    check(lib().misift_test_pyramid_layout(width, height, num_octaves, int(scale_up), off.ctypes.data, w.ctypes.data,
                                           h.ctypes.data, p.ctypes.data), "misift_test_pyramid_layout")
    return [(int(off[i]), int(w[i]), int(h[i]), int(p[i])) for i in range(num_octaves)]


def laplace_taps(num_octaves):
    k = np.zeros(8 * 12 * 16, np.float32)
    check(lib().misift_laplace_taps(num_octaves, k.ctypes.data_as(_fp)), "misift_laplace_taps")
    return k


def merge_capacity():
    """misift_test_merge_capacity (host-only): the elements of a union merge_scenes_batch stages on chip."""
    return int(lib().misift_test_merge_capacity())


def knob_names():
    """{knob: environment variable honoured under MISIFT_TUNABLES=1}."""
    return dict(kv.split("=") for kv in lib().misift_test_knob_names().decode().split(","))


def set_guard(on=True):
    """Test mode: every device allocation made from now on (DevBuf and the library's own buffers) gets 64 KiB guard bands
    and a NaN-poisoned payload (misift_test_set_guard).  Returns the previous mode."""
    return bool(lib().misift_test_set_guard(int(on)))


def check_guards():
    """Verify the guard bands of every live guarded allocation; raises MisiftError on damage, returns how many were checked."""
    n = _i(0)
    bad = lib().misift_test_check_guards(C.byref(n))
    if bad != 0:
        raise MisiftError("guard check: %d damaged allocation(s): %s" % (bad, lib().misift_last_error().decode()))
    return n.value


def select_pairs_host(recs, q, counts, offsets, stride, top, min_score, max_ambiguity, min_votes, k, max_pairs,
                      fill=0):
    """misift_test_select_pairs (host-only): misift_select_pairs_batch on host arrays by plain loops.  recs: POINT_DTYPE
    records, q: their int8 descriptors, counts / offsets (or None) / stride the layout.  Returns (sel, sel_counts, votes,
    pairs, pair_votes, summary) as int32 arrays of the stated sizes (at least one word each), pre-filled with the word
    `fill` so that unwritten entries show."""
    recs = np.ascontiguousarray(recs, POINT_DTYPE)
    q = np.ascontiguousarray(q, np.int8)
    counts = np.ascontiguousarray(counts, np.int32)
    offsets = None if offsets is None else np.ascontiguousarray(offsets, np.int32)
    n = len(counts)
    out = [np.full(max(w, 1), fill, np.uint32).view(np.int32)
           for w in (n * top, n, n * n, 2 * max_pairs, max_pairs, 8)]
    check(lib().misift_test_select_pairs(recs.ctypes.data, q.ctypes.data, n, counts.ctypes.data,
                                         None if offsets is None else offsets.ctypes.data, stride, top, min_score,
                                         max_ambiguity, min_votes, k, max_pairs, *[o.ctypes.data for o in out]),
          "misift_test_select_pairs")
    return tuple(out)


class DevBuf:
    """A raw HBM allocation owned through misift_malloc/misift_free."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib().misift_malloc(nbytes, C.byref(p)), "misift_malloc")
        self.ptr = p.value
        self.nbytes = nbytes

    def free(self):
        if self.ptr:
            lib().misift_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dptr(b):
    """A device pointer argument: a DevBuf's pointer, or a raw pointer (int or None) as given."""
    return b.ptr if isinstance(b, DevBuf) else b


def _set2(set1, set2):
    """The set-2 arguments of a batch call, both tuples from recs to stride: set 1's when recs2 is None, else set 2's
    with stride2 defaulting to stride1."""
    if set2[0] is None:
        return set1
    return set2 if set2[-1] is not None else set2[:-1] + set1[-1:]


_NO_ARGUMENT = object()                                         # _adjust_bundle: the call has no obs_weight


class Context:
    """One per device (+ optional hipStream_t given as an int)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        check(lib().misift_ctx_create(device, stream, C.byref(h)), "misift_ctx_create")
        self.h = h.value
        self.device = device

    def close(self):
        if self.h:
            lib().misift_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- options
    def get_options(self):
        o = Options()
        check(lib().misift_get_options_sized(self.h, C.byref(o), C.sizeof(o)), "misift_get_options")
        return o

    def set_options(self, **kw):
        o = self.get_options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise KeyError(k)
            setattr(o, k, int(v))
        check(lib().misift_set_options_sized(self.h, C.byref(o), C.sizeof(o)), "misift_set_options")

    def set_batches_in_flight(self, k):
        """K pipelines behind this context (misift_ctx_set_batches_in_flight): consecutive packed-async calls overlap."""
        check(lib().misift_ctx_set_batches_in_flight(self.h, k), "misift_ctx_set_batches_in_flight")

    def record_batch(self, event):
        """Record a HipEvent behind the most recently enqueued batch of this context."""
        check(lib().misift_ctx_record_batch(self.h, event.h), "misift_ctx_record_batch")

    def wait_batch(self, stream):
        """Make `stream` (a raw hipStream_t value) wait for the most recently enqueued batch of this context."""
        check(lib().misift_ctx_wait_batch(self.h, stream), "misift_ctx_wait_batch")

    def set_knob(self, name, value):
        """Developer / test knob of this context (misift_test_set_knob; capi.knob_names() lists them)."""
        check(lib().misift_test_set_knob(self.h, name.encode(), float(value)), "misift_test_set_knob")

    def test_state(self, which):
        """Host state of this context (misift_test_ctx_state; no HIP call): 0 the bytes of the shared temp, 1 the slots of
        the pinned ring of host lists, 2 the slots handed out so far."""
        v = lib().misift_test_ctx_state(self.h, which)
        if v < 0:
            raise MisiftError("misift_test_ctx_state(%d): %s" % (which, lib().misift_last_error().decode()))
        return int(v)

    def set_early_return(self, on=True):
        """Synchronous calls return at the last kernel's completion flag instead of after a stream synchronisation."""
        check(lib().misift_ctx_set_early_return(self.h, int(on)), "misift_ctx_set_early_return")

    def last_call_balanced(self):
        return lib().misift_ctx_last_call_balanced(self.h)

    def block_maps(self, cap_rows):
        """misift_test_block_maps: (orient_all's table, descr_all's table) of the last, completed call as int32 [T, 4]
        arrays; raises when that call was not balanced or holds more than cap_rows rows."""
        ta, tb = _i(0), _i(0)
        rows = np.zeros((max(cap_rows, 1), 4), np.int32)
        check(lib().misift_test_block_maps(self.h, C.byref(ta), C.byref(tb), rows.ctypes.data, cap_rows),
              "misift_test_block_maps")
        return rows[:ta.value].copy(), rows[ta.value:ta.value + tb.value].copy()

    def strip_geom(self, w, h, pitch, nframes, out_w, out_rows, out_lanes):
        """misift_test_strip_geom (no HIP call): (nstrips, seg_rows, nsegs) of a streaming launch of this context."""
        out = np.zeros(3, np.int32)
        check(lib().misift_test_strip_geom(self.h, w, h, pitch, nframes, out_w, out_rows, out_lanes, out.ctypes.data),
              "misift_test_strip_geom")
        return tuple(int(v) for v in out)

    def descr_big_fallbacks(self):
        return lib().misift_ctx_descr_big_fallbacks(self.h)

    def chain_fallbacks(self):
        return lib().misift_ctx_chain_fallbacks(self.h)

    def fuse_fallbacks(self):
        return lib().misift_ctx_fuse_fallbacks(self.h)

    def sync(self):
        check(lib().misift_ctx_sync(self.h), "misift_ctx_sync")

    def set_stream(self, stream):
        """misift_ctx_set_stream: later calls run on `stream` (a raw hipStream_t value, None for the NULL stream), behind
        everything enqueued through this context so far; no host wait."""
        check(lib().misift_ctx_set_stream(self.h, stream), "misift_ctx_set_stream")

    # ---- memory helpers
    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        buf = DevBuf(max(arr.nbytes, 16))
        if arr.nbytes:
            check(lib().misift_copy_h2d(self.h, buf.ptr, arr.ctypes.data, arr.nbytes), "misift_copy_h2d")
        return buf

    def download(self, buf, shape, dtype):
        out = np.empty(shape, dtype)
        if out.nbytes:
            check(lib().misift_copy_d2h(self.h, out.ctypes.data, buf.ptr if isinstance(buf, DevBuf) else buf,
                                        out.nbytes), "misift_copy_d2h")
        return out

    def upload_image(self, img, pitch=None):
        """Host [h,w] float32 -> pitched device image.  Returns (DevBuf, pitch_floats)."""
        img = np.ascontiguousarray(img, np.float32)
        h, w = img.shape
        if pitch is None:
            pitch = (w + 127) // 128 * 128
        buf = DevBuf(4 * pitch * h)
        check(lib().misift_upload_2d(self.h, buf.ptr, pitch, img.ctypes.data, w, w, h), "misift_upload_2d")
        return buf, pitch

    def download_image(self, ptr, w, h, pitch):
        out = np.empty((h, w), np.float32)
        check(lib().misift_download_2d(self.h, out.ctypes.data, w, ptr, pitch, w, h), "misift_download_2d")
        return out

    poison_outputs = False        # tests (guard mode): output buffers start as 0xFF instead of zero

    def zeros(self, nbytes):
        buf = DevBuf(nbytes)
        check(lib().misift_memset(self.h, buf.ptr, 0xFF if self.poison_outputs else 0, nbytes), "misift_memset")
        self.sync()
        return buf

    # ---- counters
    def get_counters(self, frame=0):
        c = (C.c_uint * 17)()
        check(lib().misift_get_counters(self.h, frame, c), "misift_get_counters")
        return np.array(list(c), np.uint32)

    def get_counter_block(self, frame=0):
        """All 64 words of a frame's counter block (diagnostic: candidate / detection / duplicate counts per octave)."""
        c = (C.c_uint * 64)()
        check(lib().misift_get_counter_block(self.h, frame, c), "misift_get_counter_block")
        return np.array(list(c), np.uint32)

    def set_counters(self, counters, frame=0):
        c = (C.c_uint * 17)(*[int(v) for v in counters])
        check(lib().misift_set_counters(self.h, frame, c), "misift_set_counters")

    # ---- stage-level calls on host arrays (upload, run, download) — used by the parity tests
    def lowpass(self, img, sigma):
        h, w = img.shape
        src, p = self.upload_image(img)
        dst = DevBuf(4 * p * h)
        check(lib().misift_lowpass(self.h, src.ptr, w, h, p, dst.ptr, p, sigma), "misift_lowpass")
        return self.download_image(dst.ptr, w, h, p)

    def scaledown(self, img):
        h, w = img.shape
        src, p = self.upload_image(img)
        w2, h2 = w // 2, h // 2
        p2 = (w2 + 127) // 128 * 128
        dst = DevBuf(4 * p2 * max(h2, 1))
        check(lib().misift_scaledown(self.h, src.ptr, w, h, p, dst.ptr, p2), "misift_scaledown")
        return self.download_image(dst.ptr, w2, h2, p2)

    def lowpass_scaledown(self, img, sigma):
        """Fused LowPass + first ScaleDown.  Returns (lowpassed [h,w], decimated [h//2,w//2])."""
        h, w = img.shape
        src, p = self.upload_image(img)
        dst = DevBuf(4 * p * h)
        w2, h2 = w // 2, h // 2
        p2 = (w2 + 127) // 128 * 128
        dst2 = DevBuf(4 * p2 * max(h2, 1))
        check(lib().misift_lowpass_scaledown(self.h, src.ptr, w, h, p, dst.ptr, p, sigma, dst2.ptr, p2),
              "misift_lowpass_scaledown")
        return self.download_image(dst.ptr, w, h, p), self.download_image(dst2.ptr, w2, h2, p2)

    def scaleup(self, img):
        h, w = img.shape
        src, p = self.upload_image(img)
        p2 = (2 * w + 127) // 128 * 128
        dst = DevBuf(4 * p2 * 2 * h)
        check(lib().misift_scaleup(self.h, src.ptr, w, h, p, dst.ptr, p2), "misift_scaleup")
        return self.download_image(dst.ptr, 2 * w, 2 * h, p2)

    def laplace(self, base, num_octaves, octave):
        h, w = base.shape
        src, p = self.upload_image(base)
        dog = DevBuf(4 * 7 * p * h)
        check(lib().misift_laplace(self.h, src.ptr, w, h, p, num_octaves, octave, dog.ptr), "misift_laplace")
        planes = self.download(dog, (7, h, p), np.float32)
        return np.ascontiguousarray(planes[:, :, :w])

    def findpoints(self, dog, thresh, subsampling=1.0, lowest_scale=0.0, max_pts=32768, octave=1,
                   edge_limit=10.0):
        """Unfused detect+refine on host DoG planes [7,h,w]. Returns (points, n)."""
        _, h, w = dog.shape
        p = (w + 127) // 128 * 128
        padded = np.zeros((7, h, p), np.float32)
        padded[:, :, :w] = dog
        d = self.upload(padded)
        pts = self.zeros(576 * max_pts)
        check(lib().misift_reset_counters(self.h, max_pts), "misift_reset_counters")
        check(lib().misift_findpoints(self.h, d.ptr, w, h, p, thresh, edge_limit, lowest_scale, subsampling,
                                      octave, pts.ptr, max_pts), "misift_findpoints")
        cnt = self.get_counters()
        n = int(min(cnt[2 * octave], max_pts))
        return self.download(pts, (max_pts,), POINT_DTYPE), n

    def dog_findpoints(self, base, num_octaves, octave, thresh, subsampling=1.0, lowest_scale=0.0,
                       max_pts=32768, edge_limit=10.0):
        """Fused DoG+detect+refine on a host base image. Returns (points, n)."""
        h, w = base.shape
        src, p = self.upload_image(base)
        pts = self.zeros(576 * max_pts)
        check(lib().misift_reset_counters(self.h, max_pts), "misift_reset_counters")
        check(lib().misift_dog_findpoints(self.h, src.ptr, w, h, p, num_octaves, octave, thresh, edge_limit,
                                          lowest_scale, subsampling, pts.ptr, max_pts), "misift_dog_findpoints")
        cnt = self.get_counters()
        n = int(min(cnt[2 * octave], max_pts))
        return self.download(pts, (max_pts,), POINT_DTYPE), n

    def orient_and_describe(self, base, pts, first, last, octave, subsampling=1.0, max_pts=None):
        """Run orientation + descriptor kernels on host points [first,last) of one octave.
        Returns (points, counters) with duplicates appended from `last`."""
        h, w = base.shape
        if max_pts is None:
            max_pts = len(pts)
        src, p = self.upload_image(base)
        d = self.upload(pts)
        cnt = np.zeros(17, np.uint32)
        cnt[2 * octave - 1] = first
        cnt[2 * octave] = last
        cnt[2 * octave + 1] = last
        check(lib().misift_reset_counters(self.h, max_pts), "misift_reset_counters")
        self.set_counters(cnt)
        check(lib().misift_orientations(self.h, src.ptr, w, h, p, octave, d.ptr, max_pts), "misift_orientations")
        check(lib().misift_descriptors(self.h, src.ptr, w, h, p, subsampling, octave, d.ptr, max_pts),
              "misift_descriptors")
        return self.download(d, (len(pts),), POINT_DTYPE), self.get_counters()

    def describe_detections_raw(self, levels, dets, pts_ptr, max_pts, scale_up=False):
        """misift_test_describe_detections on host levels and detections, records to the device pointer pts_ptr.
        levels[f][k]: the float32 image of octave k + 1 (k = 0: the coarsest level) of frame f, the last one the finest
        (its size is the call's width x height); dets[f][k]: [n, 5] float32 (xpos, ypos, scale, sharpness, edgeness).
        Returns (rc, numPts[nframes]); rc != 0 is NOT raised."""
        nframes, noct = len(levels), len(levels[0])
        h, w = levels[0][-1].shape
        lv = [np.ascontiguousarray(a, np.float32) for f in levels for a in f]
        dd = [np.ascontiguousarray(a, np.float32).reshape(-1, 5) for f in dets for a in f]
        assert len(lv) == len(dd) == nframes * noct
        ptrs = (C.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        counts = np.array([len(a) for a in dd], np.int32)
        flat = np.ascontiguousarray(np.concatenate(dd) if dd else np.zeros((0, 5), np.float32))
        n = np.full(nframes, -1, np.int32)
        rc = lib().misift_test_describe_detections(self.h, nframes, w, h, noct, int(scale_up), ptrs,
                                                   flat.ctypes.data if len(flat) else None, counts.ctypes.data, pts_ptr,
                                                   max_pts, n.ctypes.data)
        return rc, n

    def describe_detections(self, levels, dets, max_pts, scale_up=False):
        """The production per-keypoint kernels (binning, orient_all, descr_all, descr_big) on planted detections: see
        describe_detections_raw.  Returns (points[nframes, max_pts], numPts[nframes], counters[nframes, 17])."""
        nframes = len(levels)
        pts = self.zeros(576 * max_pts * nframes)
        rc, n = self.describe_detections_raw(levels, dets, pts.ptr, max_pts, scale_up)
        check(rc, "misift_test_describe_detections")
        cnt = np.stack([self.get_counters(f) for f in range(nframes)])
        return self.download(pts, (nframes, max_pts), POINT_DTYPE), n, cnt

    def detect_levels_raw(self, levels, thresh, lowest_scale, max_pts, scale_up=False, two_ranges=False):
        """misift_test_detect_levels on host levels (levels[f][k] as describe_detections_raw takes them).  Returns
        (rc, out); rc != 0 is NOT raised.  out: cand[nframes, noct, slots] uint32 and cand_counts[nframes, noct],
        dets[nframes, noct, max_pts, 5] float32 and det_counts[nframes, noct], counters[nframes, 64] uint32,
        seg_rows[noct], nstrips[noct] (index k = octave k + 1) and cand_caps[noct], the octaves' list capacities."""
        nframes, noct = len(levels), len(levels[0])
        h, w = levels[0][-1].shape
        lv = [np.ascontiguousarray(a, np.float32) for f in levels for a in f]
        assert len(lv) == nframes * noct
        ptrs = (C.c_void_p * len(lv))(*[a.ctypes.data for a in lv])
        caps = np.array([max((w >> (noct - 1 - k)) * (h >> (noct - 1 - k)) // 4, 16384) for k in range(noct)], np.int64)
        slots = int(caps.max())
        out = dict(cand=np.zeros((nframes, noct, slots), np.uint32), cand_counts=np.full((nframes, noct), -1, np.int32),
                   dets=np.zeros((nframes, noct, max(max_pts, 1), 5), np.float32),
                   det_counts=np.full((nframes, noct), -1, np.int32), counters=np.zeros((nframes, 64), np.uint32),
                   cand_caps=caps)
        geom = np.full((noct, 2), -1, np.int32)
        rc = lib().misift_test_detect_levels(self.h, nframes, w, h, noct, thresh, lowest_scale, int(scale_up), ptrs, max_pts,
                                             int(two_ranges), out["cand"].ctypes.data, slots, out["cand_counts"].ctypes.data,
                                             out["dets"].ctypes.data, out["det_counts"].ctypes.data,
                                             out["counters"].ctypes.data, geom.ctypes.data)
        out["seg_rows"], out["nstrips"] = geom[:, 0].copy(), geom[:, 1].copy()
        return rc, out

    def detect_levels(self, levels, thresh, lowest_scale=0.0, max_pts=4096, scale_up=False, two_ranges=False):
        """The production detector (dog_scan_all, refine_all) on planted pyramid levels: see detect_levels_raw."""
        rc, out = self.detect_levels_raw(levels, thresh, lowest_scale, max_pts, scale_up, two_ranges)
        check(rc, "misift_test_detect_levels")
        return out

    # ---- whole path
    def extract(self, img, num_octaves=5, init_blur=1.0, thresh=3.0, lowest_scale=0.0, scale_up=False,
                max_pts=32768, scratch=True):
        """ExtractSift on a host image.  Returns (points[max_pts], numPts, counters[17])."""
        h, w = img.shape
        src, p = self.upload_image(img)
        sc = DevBuf(4 * scratch_floats(w, h, num_octaves, scale_up)) if scratch else None
        pts = self.zeros(576 * max_pts)
        n = C.c_int(0)
        check(lib().misift_extract(self.h, src.ptr, w, h, p, num_octaves, init_blur, thresh, lowest_scale,
                                   int(scale_up), sc.ptr if sc else None, pts.ptr, max_pts, C.byref(n)),
              "misift_extract")
        return self.download(pts, (max_pts,), POINT_DTYPE), n.value, self.get_counters()

    def extract_raw(self, img_ptr, width, height, pitch, scratch_ptr, pts_ptr, num_octaves=5, init_blur=1.0, thresh=3.0,
                    lowest_scale=0.0, scale_up=False, max_pts=32768):
        """misift_extract on raw device pointers (ints): an fp32 frame at img_ptr with row stride `pitch` floats, the arena
        at scratch_ptr (None: the library's own), records to pts_ptr.  Returns (rc, numPts); rc != 0 is NOT raised."""
        n = C.c_int(-1)
        rc = lib().misift_extract(self.h, img_ptr, width, height, pitch, num_octaves, init_blur, thresh, lowest_scale,
                                  int(scale_up), scratch_ptr, pts_ptr, max_pts, C.byref(n))
        return rc, n.value

    def extract_batch_raw(self, imgs_ptr, src_u8, nframes, frame_stride, width, height, pitch, scratch_ptr, pts_ptr,
                          num_octaves=5, init_blur=1.0, thresh=3.0, lowest_scale=0.0, scale_up=False, max_pts=32768):
        """misift_extract_batch_ex on raw device pointers (ints): 8-bit or fp32 frames, pitch and frame_stride in source
        elements.  Returns (rc, numPts[nframes]); rc != 0 is NOT raised."""
        n = (C.c_int * nframes)(*([-1] * nframes))
        rc = lib().misift_extract_batch_ex(self.h, imgs_ptr, int(src_u8), nframes, frame_stride, width, height, pitch,
                                           num_octaves, init_blur, thresh, lowest_scale, int(scale_up), scratch_ptr,
                                           pts_ptr, max_pts, n)
        return rc, np.array(list(n), np.int32)

    def extract_batch_packed_async_raw(self, imgs_ptr, nframes, frame_stride, width, height, pitch, scratch_ptr, pts_ptr,
                                       counts_ptr, offsets_ptr, packed_ptr, num_octaves=5, init_blur=1.0, thresh=3.0,
                                       lowest_scale=0.0, max_pts=32768):
        """misift_extract_batch_packed_async on raw device pointers (ints); enqueued on the context stream.  Returns rc
        (not raised)."""
        return lib().misift_extract_batch_packed_async(self.h, imgs_ptr, nframes, frame_stride, width, height, pitch,
                                                       num_octaves, init_blur, thresh, lowest_scale, scratch_ptr, pts_ptr,
                                                       max_pts, counts_ptr, offsets_ptr, packed_ptr)

    def extract_batch(self, imgs, num_octaves=5, init_blur=1.0, thresh=3.0, lowest_scale=0.0, max_pts=32768):
        """imgs: [B,h,w] host array.  Returns (points[B,max_pts], numPts[B])."""
        imgs = np.ascontiguousarray(imgs, np.float32)
        B, h, w = imgs.shape
        p = (w + 127) // 128 * 128
        padded = np.zeros((B, h, p), np.float32)
        padded[:, :, :w] = imgs
        d = self.upload(padded)
        S = scratch_floats(w, h, num_octaves, False)
        sc = DevBuf(4 * S * B)
        pts = self.zeros(576 * max_pts * B)
        n = (C.c_int * B)()
        check(lib().misift_extract_batch(self.h, d.ptr, B, h * p, w, h, p, num_octaves, init_blur, thresh,
                                         lowest_scale, sc.ptr, pts.ptr, max_pts, n), "misift_extract_batch")
        return self.download(pts, (B, max_pts), POINT_DTYPE), np.array(list(n), np.int32)

    def extract_batch_ex(self, imgs, num_octaves=5, init_blur=1.0, thresh=3.0, lowest_scale=0.0, scale_up=False,
                         max_pts=32768):
        """imgs: [B,h,w] uint8 or float32 host array (tightly packed).  Returns (points[B,max_pts], numPts[B])."""
        u8 = imgs.dtype == np.uint8
        imgs = np.ascontiguousarray(imgs, np.uint8 if u8 else np.float32)
        B, h, w = imgs.shape
        d = self.upload(imgs)
        sc = DevBuf(4 * scratch_floats(w, h, num_octaves, scale_up) * B)
        pts = self.zeros(576 * max_pts * B)
        n = (C.c_int * B)()
        check(lib().misift_extract_batch_ex(self.h, d.ptr, int(u8), B, h * w, w, h, w, num_octaves, init_blur, thresh,
                                            lowest_scale, int(scale_up), sc.ptr, pts.ptr, max_pts, n),
              "misift_extract_batch_ex")
        return self.download(pts, (B, max_pts), POINT_DTYPE), np.array(list(n), np.int32)

    def extract_batch_u8(self, imgs, num_octaves=5, init_blur=1.0, thresh=3.0, lowest_scale=0.0, max_pts=32768):
        """imgs: [B,h,w] uint8 host array (tightly packed).  Returns (points[B,max_pts], numPts[B])."""
        imgs = np.ascontiguousarray(imgs, np.uint8)
        B, h, w = imgs.shape
        d = self.upload(imgs)
        S = scratch_floats(w, h, num_octaves, False)
        sc = DevBuf(4 * S * B)
        pts = self.zeros(576 * max_pts * B)
        n = (C.c_int * B)()
        check(lib().misift_extract_batch_u8(self.h, d.ptr, B, h * w, w, h, w, num_octaves, init_blur, thresh,
                                            lowest_scale, sc.ptr, pts.ptr, max_pts, n), "misift_extract_batch_u8")
        return self.download(pts, (B, max_pts), POINT_DTYPE), np.array(list(n), np.int32)

    def match(self, pts1, n1, pts2, n2, row_begin=0, row_count=None):
        """MatchSiftData on host structured arrays; returns the updated copy of pts1."""
        d1 = self.upload(pts1)
        d2 = self.upload(pts2)
        if row_count is None:
            check(lib().misift_match(self.h, d1.ptr, n1, d2.ptr, n2), "misift_match")
        else:
            check(lib().misift_match_rows(self.h, d1.ptr, row_begin, row_count, d2.ptr, n2), "misift_match_rows")
        return self.download(d1, (len(pts1),), POINT_DTYPE)

    def match_batch(self, pairs, recs1, nframes1, counts1, offsets1=None, stride1=0, recs2=None, nframes2=None,
                    counts2=None, offsets2=None, stride2=None):
        """misift_match_batch: for each row (f1, f2) of `pairs`, MatchSiftData of frame f1 of set 1 against frame f2 of
        set 2, on device buffers (DevBuf or raw device pointers).  Frame f of a set holds max(counts[f], 0) records from
        record offsets[f] (offsets None: f * stride).  Set 2 defaults to set 1 (frame f against frame f + 1 of one
        batch).  Enqueued on the context stream: the results are there once sync() (or later stream work) has run."""
        recs2, nframes2, counts2, offsets2, stride2 = _set2((recs1, nframes1, counts1, offsets1, stride1),
                                                            (recs2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        check(lib().misift_match_batch(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), nframes1,
                                       _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2), nframes2,
                                       _dptr(counts2), _dptr(offsets2), stride2), "misift_match_batch")

    def match_pairs_batch(self, pairs, recs1, nframes1, counts1, offsets1=None, stride1=0, recs2=None, nframes2=None,
                          counts2=None, offsets2=None, stride2=None, max_pts=8192, mutual=False, out=None,
                          out_counts=None, num_matched=None):
        """misift_match_pairs_batch: match_batch into pair-indexed output rows — row r of pair i is the record
        out[i * max_pts + r] (device, npairs * max_pts records, allocated here when None) — so frames may repeat across
        pairs; with `mutual` only rows that are also their match's best row keep the match.  Frames and the set-2
        default as in match_batch.  out_counts (npairs ints: n1, or -1 over max_pts) and num_matched (npairs ints: rows
        with match >= 0, -1 over max_pts) are device buffers, allocated here when None; returns (out, out_counts,
        num_matched).  Enqueued on the context stream."""
        recs2, nframes2, counts2, offsets2, stride2 = _set2((recs1, nframes1, counts1, offsets1, stride1),
                                                            (recs2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = max(len(pairs), 1)
        if out is None:
            out = self.zeros(POINT_DTYPE.itemsize * n * max(max_pts, 1))
        if out_counts is None:
            out_counts = self.zeros(4 * n)
        if num_matched is None:
            num_matched = self.zeros(4 * n)
        check(lib().misift_match_pairs_batch(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), nframes1,
                                             _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2), nframes2,
                                             _dptr(counts2), _dptr(offsets2), stride2, max_pts, int(mutual),
                                             _dptr(out), _dptr(out_counts), _dptr(num_matched)),
              "misift_match_pairs_batch")
        return out, out_counts, num_matched

    def find_homography_batch(self, frames, seeds, recs, nframes, counts, offsets=None, stride=0, max_pts=8192,
                              num_loops=1000, min_score=0.85, max_ambiguity=0.95, thresh=5.0, homography=None,
                              num_matches=None):
        """misift_find_homography_batch: FindHomography of frame frames[i] of a device-resident record batch, as after
        srand(seeds[i]), into slot i of the device buffers `homography` (nsel x 9 floats) and `num_matches` (nsel ints),
        allocated here when None and returned.  Frames as in match_batch.  Enqueued on the context stream: the results
        are there once sync() (or later stream work) has run."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        assert len(seeds) == len(frames)
        if homography is None:
            homography = self.zeros(4 * 9 * max(len(frames), 1))
        if num_matches is None:
            num_matches = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_find_homography_batch(self.h, len(frames), frames.ctypes.data, seeds.ctypes.data,
                                                 _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride, max_pts,
                                                 num_loops, min_score, max_ambiguity, thresh, _dptr(homography),
                                                 _dptr(num_matches)),
              "misift_find_homography_batch")
        return homography, num_matches

    def improve_homography_batch(self, frames, recs, nframes, counts, homography, offsets=None, stride=0, num_fit=None,
                                 num_loops=5, min_score=0.0, max_ambiguity=0.80, thresh=3.0):
        """misift_improve_homography_batch: ImproveHomography of frame frames[i] from the start homography[9i..9i+8]
        (device, refined in place), writing match_error of the frame's records and num_fit[i] (device, nsel ints,
        allocated here when None and returned).  Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        if num_fit is None:
            num_fit = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_improve_homography_batch(self.h, len(frames), frames.ctypes.data, _dptr(recs), nframes,
                                                    _dptr(counts), _dptr(offsets), stride, num_loops, min_score,
                                                    max_ambiguity, thresh, _dptr(homography), _dptr(num_fit)),
              "misift_improve_homography_batch")
        return num_fit

    def find_fundamental_batch(self, frames, seeds, recs, nframes, counts, offsets=None, stride=0, max_pts=8192,
                               num_loops=1000, min_score=0.85, max_ambiguity=0.95, thresh=1.0, fundamental=None,
                               num_inliers=None):
        """misift_find_fundamental_batch: a RANSAC fundamental matrix (normalised 8-point samples drawn from seeds[i],
        inliers by Sampson distance < thresh) of the stored matches of frame frames[i] of a device-resident record
        batch, into slot i of the device buffers `fundamental` (nsel x 9 floats, (x2, y2, 1) F (x1, y1, 1)^T = 0) and
        `num_inliers` (nsel ints; -1 over max_pts), allocated here when None and returned.  Frames as in match_batch.
        Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        assert len(seeds) == len(frames)
        if fundamental is None:
            fundamental = self.zeros(4 * 9 * max(len(frames), 1))
        if num_inliers is None:
            num_inliers = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_find_fundamental_batch(self.h, len(frames), frames.ctypes.data, seeds.ctypes.data,
                                                  _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride, max_pts,
                                                  num_loops, min_score, max_ambiguity, thresh, _dptr(fundamental),
                                                  _dptr(num_inliers)),
              "misift_find_fundamental_batch")
        return fundamental, num_inliers

    def score_fundamental_batch(self, frames, recs, nframes, counts, fundamental, offsets=None, stride=0, num_fit=None,
                                min_score=0.85, max_ambiguity=0.95, thresh=1.0):
        """misift_score_fundamental_batch: the Sampson distance of every record of frame frames[i] under
        fundamental[9i..9i+8] (device, e.g. find_fundamental_batch's result) into its match_error, which
        link_tracks_batch gates on through max_error; num_fit[i] (device, nsel ints, allocated here when None and
        returned) = the records that pass the gates and lie within thresh.  Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        if num_fit is None:
            num_fit = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_score_fundamental_batch(self.h, len(frames), frames.ctypes.data, _dptr(recs), nframes,
                                                   _dptr(counts), _dptr(offsets), stride, min_score, max_ambiguity,
                                                   thresh, _dptr(fundamental), _dptr(num_fit)),
              "misift_score_fundamental_batch")
        return num_fit

    def improve_fundamental_batch(self, frames, recs, nframes, counts, fundamental, offsets=None, stride=0,
                                  num_fit=None, num_rounds=None, num_loops=5, min_score=0.85, max_ambiguity=0.95,
                                  thresh=1.0):
        """misift_improve_fundamental_batch: up to num_loops refits of fundamental[9i..9i+8] (device, e.g.
        find_fundamental_batch's result, refined in place) over the records of frame frames[i] that pass the gates and lie
        within thresh of it, each kept only if it loses no inlier; then match_error of every record of the frame under
        the result, as score_fundamental_batch writes it (num_loops = 0 is that call).  num_fit[i] (device, nsel ints,
        allocated here when None and returned) = the inliers of the result; num_rounds (device, nsel ints, optional) =
        the refits kept.  Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        if num_fit is None:
            num_fit = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_improve_fundamental_batch(self.h, len(frames), frames.ctypes.data, _dptr(recs), nframes,
                                                     _dptr(counts), _dptr(offsets), stride, num_loops, min_score,
                                                     max_ambiguity, thresh, _dptr(fundamental), _dptr(num_fit),
                                                     _dptr(num_rounds)),
              "misift_improve_fundamental_batch")
        return num_fit

    def recover_pose_batch(self, frames, intrinsics, recs, nframes, counts, fundamental, offsets=None, stride=0,
                           pose=None, num_front=None, votes=None, xyz=None, min_score=0.85, max_ambiguity=0.95,
                           thresh=1.0):
        """misift_recover_pose_batch: the relative pose X2 = R X1 + t, |t| = 1, of frame frames[i] from
        fundamental[9i..9i+8] (device, e.g. improve_fundamental_batch's result) and intrinsics[i] = fx1 fy1 cx1 cy1 fx2
        fy2 cx2 cy2 (host, nsel x 8): the decomposition of E = K2^T F K1 that puts the most records that pass the gates
        and lie within thresh of F in front of both cameras.  pose (device, nsel x 12 floats: R row-major, then t) and
        num_front (device, nsel ints: the winner's vote) are allocated here when None and returned.  votes (device, nsel
        x 4 ints) and xyz (device, 4 floats per record of `recs`, indexed like it: the point in camera 1 and its depth in
        camera 2) are optional.  The records are not written.  Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 8)
        assert len(intrinsics) == len(frames)
        if pose is None:
            pose = self.zeros(4 * 12 * max(len(frames), 1))
        if num_front is None:
            num_front = self.zeros(4 * max(len(frames), 1))
        check(lib().misift_recover_pose_batch(self.h, len(frames), frames.ctypes.data, intrinsics.ctypes.data,
                                              _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride, min_score,
                                              max_ambiguity, thresh, _dptr(fundamental), _dptr(pose), _dptr(num_front),
                                              _dptr(votes), _dptr(xyz)),
              "misift_recover_pose_batch")
        return pose, num_front

    def recover_pose_planar_batch(self, frames, intrinsics, recs, nframes, counts, homography, fundamental=None,
                                  offsets=None, stride=0, model=None, hf_counts=None, pose=None, num_front=None,
                                  votes=None, xyz=None, pose_alt=None, plane=None, min_score=0.85, max_ambiguity=0.95,
                                  thresh_h=1.0, thresh_f=1.0, planar_ratio=0.8, min_inliers=8, min_baseline=0.02):
        """misift_recover_pose_planar_batch: behind recover_pose_batch, the pose of every frame frames[i] whose matches
        lie on one plane (model 1) or whose camera only rotates (model 2), from homography[9i..9i+8] (device, set-1 to
        set-2 pixels, e.g. improve_homography_batch's result) and intrinsics[i] (host, nsel x 8).  With fundamental
        (device, nsel x 9) an entry is a candidate when its H-inliers at thresh_h number at least min_inliers and
        planar_ratio times its F-inliers at thresh_f; without it, min_inliers alone decides.  pose, num_front, votes and
        xyz are recover_pose_batch's own buffers: entries of model 1 and 2 are overwritten, all others are left alone
        (pose and num_front are allocated here when None).  model (device, nsel ints: -1, 0, 1, 2) and hf_counts
        (device, nsel x 2 ints: nH, nF) are allocated here when None; pose_alt (device, nsel x 12: the other rotation's
        better hypothesis) and plane (device, nsel x 4: N in camera 1 and d in units of |t|) are optional.  Returns
        (model, hf_counts, pose, num_front).  The thresholds default to 1 px as `thresh` does in every sibling wrapper, so
        the chain's calls agree when none is given; planar_ratio and min_baseline default to the header's 0.8 and 0.02.
        The records are not written.  Enqueued on the context stream."""
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 8)
        assert len(intrinsics) == len(frames)
        ns = max(len(frames), 1)
        if model is None:
            model = self.zeros(4 * ns)
        if hf_counts is None:
            hf_counts = self.zeros(4 * 2 * ns)
        if pose is None:
            pose = self.zeros(4 * 12 * ns)
        if num_front is None:
            num_front = self.zeros(4 * ns)
        check(lib().misift_recover_pose_planar_batch(self.h, len(frames), frames.ctypes.data, intrinsics.ctypes.data,
                                                     _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride,
                                                     min_score, max_ambiguity, thresh_h, thresh_f, planar_ratio,
                                                     min_inliers, min_baseline, _dptr(homography), _dptr(fundamental),
                                                     _dptr(model), _dptr(hf_counts), _dptr(pose), _dptr(num_front),
                                                     _dptr(votes), _dptr(xyz), _dptr(pose_alt), _dptr(plane)),
              "misift_recover_pose_planar_batch")
        return model, hf_counts, pose, num_front

    def link_poses_batch(self, pairs, nimages, rows, row_counts, max_pts, pose, num_front, xyz, links, seed_pair,
                         root_image, walk, min_common=8, link_ratio=None, link_common=None, pair_scale=None, cam=None,
                         cam_pair=None, summary=None, min_score=0.85, max_ambiguity=0.95, max_error=float("inf")):
        """misift_link_poses_batch: the pair poses of recover_pose_batch (pose, num_front, xyz for the rows of
        match_pairs_batch, frame i = pair i) joined into one frame.  links (host, nlinks x 3: p, q, kind with 0 = CHAIN,
        p's set-2 image is q's set-1 image, 1 = FAN, the same set-1 image) each get the lower median of the depth ratios of
        their common points; the scales spread from seed_pair over the links in the order given; walk (host, pair
        indices) places a camera X_i = R_i X_world + t_i per image from root_image on.  The six outputs (device:
        link_ratio and link_common per link, pair_scale per pair, cam nimages x 12, cam_pair per image, summary 8 ints)
        are allocated here when None and returned in that order.  Enqueued on the context stream."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        links = np.ascontiguousarray(links, np.int32).reshape(-1, 3)
        walk = np.ascontiguousarray(walk, np.int32).reshape(-1)
        if link_ratio is None:
            link_ratio = self.zeros(4 * max(len(links), 1))
        if link_common is None:
            link_common = self.zeros(4 * max(len(links), 1))
        if pair_scale is None:
            pair_scale = self.zeros(4 * max(len(pairs), 1))
        if cam is None:
            cam = self.zeros(4 * 12 * max(nimages, 1))
        if cam_pair is None:
            cam_pair = self.zeros(4 * max(nimages, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_link_poses_batch(self.h, len(pairs), pairs.ctypes.data, nimages, _dptr(rows),
                                            _dptr(row_counts), max_pts, min_score, max_ambiguity, max_error,
                                            _dptr(pose), _dptr(num_front), _dptr(xyz), len(links), links.ctypes.data,
                                            seed_pair, root_image, min_common, len(walk), walk.ctypes.data,
                                            _dptr(link_ratio), _dptr(link_common), _dptr(pair_scale), _dptr(cam),
                                            _dptr(cam_pair), _dptr(summary)),
              "misift_link_poses_batch")
        return link_ratio, link_common, pair_scale, cam, cam_pair, summary

    def match_guided_batch(self, pairs, recs1, nframes1, counts1, homography, radius, offsets1=None, stride1=0,
                           recs2=None, nframes2=None, counts2=None, offsets2=None, stride2=None, max_pts=8192,
                           num_found=None):
        """misift_match_guided_batch: for each row (f1, f2) of `pairs`, every record of frame f1 of set 1 matched against
        the records of frame f2 of set 2 within `radius` of its projection through homography[9i..9i+8] (device, npairs
        x 9 floats, e.g. find_homography_batch's result).  Frames and the set-2 default as in match_batch.  Writes
        num_found (device, npairs ints, allocated here when None and returned): rows matched, 0 for an empty side, -1
        over max_pts.  Enqueued on the context stream."""
        recs2, nframes2, counts2, offsets2, stride2 = _set2((recs1, nframes1, counts1, offsets1, stride1),
                                                            (recs2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        if num_found is None:
            num_found = self.zeros(4 * max(len(pairs), 1))
        check(lib().misift_match_guided_batch(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), nframes1,
                                              _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2), nframes2,
                                              _dptr(counts2), _dptr(offsets2), stride2, _dptr(homography), radius,
                                              max_pts, _dptr(num_found)), "misift_match_guided_batch")
        return num_found

    def match_epipolar_batch(self, pairs, recs1, nframes1, counts1, fundamental, radius, offsets1=None, stride1=0,
                             recs2=None, nframes2=None, counts2=None, offsets2=None, stride2=None, max_pts=8192,
                             num_found=None):
        """misift_match_epipolar_batch: for each row (f1, f2) of `pairs`, every record of frame f1 of set 1 matched
        against the records of frame f2 of set 2 within `radius` of its epipolar line under fundamental[9i..9i+8] (device,
        npairs x 9 floats, (x2, y2, 1) F (x1, y1, 1)^T = 0, e.g. find_fundamental_batch's result).  Frames, the set-2
        default and num_found as in match_guided_batch.  Enqueued on the context stream."""
        recs2, nframes2, counts2, offsets2, stride2 = _set2((recs1, nframes1, counts1, offsets1, stride1),
                                                            (recs2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        if num_found is None:
            num_found = self.zeros(4 * max(len(pairs), 1))
        check(lib().misift_match_epipolar_batch(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), nframes1,
                                                _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2), nframes2,
                                                _dptr(counts2), _dptr(offsets2), stride2, _dptr(fundamental), radius,
                                                max_pts, _dptr(num_found)), "misift_match_epipolar_batch")
        return num_found

    def quantize_batch(self, recs, nframes, counts, offsets=None, stride=0, q=None):
        """misift_quantize_batch: the 8-bit descriptors of every record of every frame (frames as in match_batch) into
        `q` (device, 128 bytes per record index, 16-byte aligned; allocated here for the records of the largest index a
        frame can reach when None: pass q for packed layouts whose total only the device knows).  Returns q.  Enqueued
        on the context stream."""
        if q is None:
            assert isinstance(recs, DevBuf), "pass q when recs is a raw pointer"
            q = self.zeros(max(128 * (recs.nbytes // 576), 16))
        check(lib().misift_quantize_batch(self.h, _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride,
                                          _dptr(q)),
              "misift_quantize_batch")
        return q

    def match_batch_i8(self, pairs, recs1, q1, nframes1, counts1, offsets1=None, stride1=0, recs2=None, q2=None,
                       nframes2=None, counts2=None, offsets2=None, stride2=None):
        """misift_match_batch_i8: match_batch on the 8-bit descriptors q1 / q2 (quantize_batch's output for recs1 /
        recs2) on the int8 matrix cores.  Set 2 defaults to set 1.  Enqueued on the context stream."""
        recs2, q2, nframes2, counts2, offsets2, stride2 = _set2((recs1, q1, nframes1, counts1, offsets1, stride1),
                                                                (recs2, q2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        check(lib().misift_match_batch_i8(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), _dptr(q1), nframes1,
                                          _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2), _dptr(q2), nframes2,
                                          _dptr(counts2), _dptr(offsets2), stride2),
              "misift_match_batch_i8")

    def match_pairs_batch_i8(self, pairs, recs1, q1, nframes1, counts1, offsets1=None, stride1=0, recs2=None, q2=None,
                             nframes2=None, counts2=None, offsets2=None, stride2=None, max_pts=8192, mutual=False,
                             out=None, out_counts=None, num_matched=None):
        """misift_match_pairs_batch_i8: match_pairs_batch with the scores of match_batch_i8 — pair-indexed output rows
        (row r of pair i is out[i * max_pts + r]) from the 8-bit descriptors q1 / q2 (quantize_batch's output for recs1
        / recs2), so frames may repeat across pairs; with `mutual` only rows that are also their match's best row keep
        the match.  Set 2 (records and q) defaults to set 1.  out, out_counts and num_matched as in match_pairs_batch:
        device buffers, allocated here when None; returns (out, out_counts, num_matched).  Enqueued on the context
        stream."""
        recs2, q2, nframes2, counts2, offsets2, stride2 = _set2((recs1, q1, nframes1, counts1, offsets1, stride1),
                                                                (recs2, q2, nframes2, counts2, offsets2, stride2))
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = max(len(pairs), 1)
        if out is None:
            out = self.zeros(POINT_DTYPE.itemsize * n * max(max_pts, 1))
        if out_counts is None:
            out_counts = self.zeros(4 * n)
        if num_matched is None:
            num_matched = self.zeros(4 * n)
        check(lib().misift_match_pairs_batch_i8(self.h, len(pairs), pairs.ctypes.data, _dptr(recs1), _dptr(q1),
                                                nframes1, _dptr(counts1), _dptr(offsets1), stride1, _dptr(recs2),
                                                _dptr(q2), nframes2, _dptr(counts2), _dptr(offsets2), stride2, max_pts,
                                                int(mutual), _dptr(out), _dptr(out_counts), _dptr(num_matched)),
              "misift_match_pairs_batch_i8")
        return out, out_counts, num_matched

    def select_pairs_batch(self, recs, q, nframes, counts, offsets=None, stride=0, top=256, min_score=0.85,
                           max_ambiguity=0.95, min_votes=4, k=8, max_pairs=None, sel=None, sel_counts=None, votes=None,
                           pairs=None, pair_votes=None, summary=None):
        """misift_select_pairs_batch (preemptive matching): the frame pairs worth matching.  The `top` largest-scale
        records of every frame (q: quantize_batch's output for recs) are matched against those of every other frame,
        votes[a, b] counts the mutual matches that pass the gate (min_score, max_ambiguity), every frame takes its k
        best partners with at least min_votes votes, and the selected pairs (a < b) are written in ascending order
        while they fit max_pairs (default: every pair).  sel (nframes x top ints), sel_counts (nframes), votes (nframes
        x nframes), pairs (2 x max_pairs), pair_votes (max_pairs) and summary (8 ints: pairs selected, pairs written,
        frames without neighbour, frames with more than top records, max votes) are device buffers, allocated here
        when None; returns the six.  Enqueued on the context stream; read_selected_pairs() is the host step."""
        if max_pairs is None:
            max_pairs = nframes * (nframes - 1) // 2
        n = max(nframes, 1)
        if sel is None:
            sel = self.zeros(4 * n * max(top, 1))
        if sel_counts is None:
            sel_counts = self.zeros(4 * n)
        if votes is None:
            votes = self.zeros(4 * n * n)
        if pairs is None:
            pairs = self.zeros(8 * max(max_pairs, 1))
        if pair_votes is None:
            pair_votes = self.zeros(4 * max(max_pairs, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_select_pairs_batch(self.h, _dptr(recs), _dptr(q), nframes, _dptr(counts), _dptr(offsets),
                                              stride, top, min_score, max_ambiguity, min_votes, k, max_pairs, _dptr(sel),
                                              _dptr(sel_counts), _dptr(votes), _dptr(pairs), _dptr(pair_votes),
                                              _dptr(summary)), "misift_select_pairs_batch")
        return sel, sel_counts, votes, pairs, pair_votes, summary

    def read_selected_pairs(self, pairs, summary):
        """The host step behind select_pairs_batch: waits for the stream and returns the written pairs as the (n, 2)
        int32 host array the pair matchers take."""
        s = self.download(summary, (8,), np.int32)
        n = int(s[1])
        if n == 0:
            return np.zeros((0, 2), np.int32)
        return self.download(pairs, (n, 2), np.int32)

    def link_tracks_batch(self, pairs, rows, row_counts, max_pts, nframes, counts, offsets=None, stride=0,
                          max_records=None, min_score=0.85, max_ambiguity=0.95, max_error=float("inf"), track=None,
                          track_len=None, track_frames=None, summary=None):
        """misift_link_tracks_batch: the accepted matches of a pair-indexed batch (`rows`, `row_counts`, `max_pts`:
        match_pairs_batch's out, out_counts and max_pts for `pairs`) joined across pairs into feature tracks over the
        global record indices of the one record batch (nframes, counts, offsets or stride) both frames of every pair
        belong to.  A row is an edge when its match is a record of frame f2, score > min_score, ambiguity <
        max_ambiguity and, with a finite max_error, match_error < max_error.  track, track_len, track_frames
        (max_records ints each, mirroring the record indices) and summary (8 ints) are device buffers, allocated here
        when None; returns the four.  Enqueued on the context stream."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        assert max_records is not None, "max_records: the length of the record index space"
        n = 4 * max(max_records, 1)
        if track is None:
            track = self.zeros(n)
        if track_len is None:
            track_len = self.zeros(n)
        if track_frames is None:
            track_frames = self.zeros(n)
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_link_tracks_batch(self.h, len(pairs), pairs.ctypes.data if len(pairs) else None,
                                             _dptr(rows), _dptr(row_counts), max_pts, nframes, _dptr(counts),
                                             _dptr(offsets), stride, max_records, min_score, max_ambiguity, max_error,
                                             _dptr(track), _dptr(track_len), _dptr(track_frames), _dptr(summary)),
              "misift_link_tracks_batch")
        return track, track_len, track_frames, summary

    def export_tracks_batch(self, recs, nframes, counts, offsets=None, stride=0, max_records=None, track=None,
                            track_len=None, track_frames=None, min_len=2, consistent_only=True, max_tracks=None,
                            max_obs=None, track_offsets=None, track_root=None, obs=None, record_obs=True, summary=None):
        """misift_export_tracks_batch: the labels link_tracks_batch wrote (track, track_len, track_frames, for the same
        layout and max_records) as compact observation lists.  The roots with track_len >= min_len (and, with
        consistent_only, track_len == track_frames) are numbered in ascending order; track t's observations
        (TRACK_OBS_DTYPE: frame, record, xpos, ypos) are obs[track_offsets[t]:track_offsets[t + 1]], in ascending order
        of the global index; a track that does not fit max_tracks / max_obs (default: max_records each) is left out
        whole, with everything behind it.  track_offsets (max_tracks + 1 ints), track_root (max_tracks ints), obs
        (max_obs entries), record_obs (max_records ints: each record's slot in obs or -1; True allocates it, None
        leaves it out) and summary (8 ints) are device buffers, allocated here when not passed; returns the five.
        Enqueued on the context stream."""
        assert max_records is not None, "max_records: the length of the record index space"
        max_tracks = max_records if max_tracks is None else max_tracks
        max_obs = max_records if max_obs is None else max_obs
        if track_offsets is None:
            track_offsets = self.zeros(4 * (max(max_tracks, 1) + 1))
        if track_root is None:
            track_root = self.zeros(4 * max(max_tracks, 1))
        if obs is None:
            obs = self.zeros(TRACK_OBS_DTYPE.itemsize * max(max_obs, 1))
        if record_obs is True:
            record_obs = self.zeros(4 * max(max_records, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_export_tracks_batch(self.h, _dptr(recs), nframes, _dptr(counts), _dptr(offsets), stride,
                                               max_records, _dptr(track), _dptr(track_len), _dptr(track_frames),
                                               min_len, int(consistent_only), max_tracks, max_obs,
                                               _dptr(track_offsets), _dptr(track_root), _dptr(obs), _dptr(record_obs),
                                               _dptr(summary)), "misift_export_tracks_batch")
        return track_offsets, track_root, obs, record_obs, summary

    def triangulate_tracks_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, nimages, cam, cam_pair,
                                 intrinsics, min_views=2, num_loops=5, points=None, point_views=None,
                                 point_status=None, obs_error=True, summary=None):
        """misift_triangulate_tracks_batch: one world point per track that export_tracks_batch wrote (track_offsets, obs,
        export_summary: its outputs for max_tracks and max_obs) under the cameras of link_poses_batch (cam, cam_pair, for
        nimages images; obs.frame is the image index) and intrinsics (host, nimages x 4: fx fy cx cy).  A linear start
        over the views whose image has a camera, then up to num_loops Gauss-Newton steps on the reprojection error, each
        kept only if it lowers it.  points (max_tracks x 4 floats: X Y Z in the world frame, rms reprojection error in
        px), point_views and point_status (max_tracks ints: the views used; 0 ok, 1 fewer than min_views, 2 singular, 3
        behind a camera, 4 a bad range), obs_error (max_obs floats: each observation's residual in px; True allocates
        it, None leaves it out) and summary (8 ints) are device buffers, allocated here when not passed; returns the
        five.  Enqueued on the context stream."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        if points is None:
            points = self.zeros(16 * max(max_tracks, 1))
        if point_views is None:
            point_views = self.zeros(4 * max(max_tracks, 1))
        if point_status is None:
            point_status = self.zeros(4 * max(max_tracks, 1))
        if obs_error is True:
            obs_error = self.zeros(4 * max(max_obs, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_triangulate_tracks_batch(self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs),
                                                    _dptr(export_summary), nimages, _dptr(cam), _dptr(cam_pair),
                                                    intrinsics.ctypes.data, min_views, num_loops, _dptr(points),
                                                    _dptr(point_views), _dptr(point_status), _dptr(obs_error),
                                                    _dptr(summary)), "misift_triangulate_tracks_batch")
        return points, point_views, point_status, obs_error, summary

    def refine_cameras_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                             nimages, cam, cam_pair, intrinsics, hold=(), min_obs=6, num_loops=5, max_error=np.inf,
                             orthonormalise=True, cam_out=None, cam_obs=None, cam_rms=None, cam_steps=None,
                             cam_status=None, summary=None):
        """misift_refine_cameras_batch: every camera of link_poses_batch (cam, cam_pair, for nimages images) moved to
        minimise the reprojection error of the observations its image makes (track_offsets, obs, export_summary: the
        outputs of export_tracks_batch for max_tracks and max_obs) of the points of triangulate_tracks_batch (points,
        point_status), the points held.  intrinsics: host, nimages x 4 (fx fy cx cy); hold: host, the images kept as
        they are besides the root.  The rotation is re-orthonormalised first when orthonormalise is set; an observation
        is used when its point is in front and within max_error px; an image with fewer than min_obs of them keeps its
        camera; then up to num_loops Gauss-Newton steps, each kept only if it lowers the error.  cam_out (nimages x 12
        floats; may be cam itself), cam_obs, cam_steps and cam_status (nimages ints: the observations used, the steps
        kept; 0 ok, 1 fewer than min_obs, 2 singular, 3 root or held, 4 no camera), cam_rms (nimages x 2 floats: rms
        reprojection error in px before and after) and summary (8 ints) are device buffers, allocated here when not
        passed; returns the six.  Enqueued on the context stream."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        hold = np.ascontiguousarray(hold, np.int32).reshape(-1)
        if cam_out is None:
            cam_out = self.zeros(48 * max(nimages, 1))
        if cam_obs is None:
            cam_obs = self.zeros(4 * max(nimages, 1))
        if cam_rms is None:
            cam_rms = self.zeros(8 * max(nimages, 1))
        if cam_steps is None:
            cam_steps = self.zeros(4 * max(nimages, 1))
        if cam_status is None:
            cam_status = self.zeros(4 * max(nimages, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_refine_cameras_batch(self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs),
                                                _dptr(export_summary), _dptr(points), _dptr(point_status), nimages,
                                                _dptr(cam), _dptr(cam_pair), intrinsics.ctypes.data, len(hold),
                                                hold.ctypes.data if len(hold) else None, int(min_obs), int(num_loops),
                                                float(max_error), int(orthonormalise), _dptr(cam_out), _dptr(cam_obs),
                                                _dptr(cam_rms), _dptr(cam_steps), _dptr(cam_status), _dptr(summary)),
              "misift_refine_cameras_batch")
        return cam_out, cam_obs, cam_rms, cam_steps, cam_status, summary

    def adjust_bundle_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                            nimages, cam, cam_pair, intrinsics, hold=(), min_views=2, min_obs=6, num_loops=5,
                            cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=True, cam_out=None,
                            points_out=None, cam_obs=None, cam_status=None, cam_rms=None, point_obs=None, history=None,
                            cost=None, summary=None):
        """misift_adjust_bundle_batch: the cameras (cam, cam_pair, for nimages images) and the points of
        triangulate_tracks_batch (points, point_status) adjusted jointly against the observations (track_offsets, obs,
        export_summary: the outputs of export_tracks_batch for max_tracks and max_obs): num_loops Levenberg-Marquardt
        steps from damping lambda0, the points eliminated in each, the cameras solved by cg_iters preconditioned
        conjugate-gradient iterations, each step kept only if it lowers the error.  intrinsics: host, nimages x 4 (fx fy
        cx cy); hold: host, the images kept as they are besides the root.  An observation is used when its point is in
        front and within max_error px; a track with fewer than min_views of them keeps its point, a camera with fewer
        than min_obs stays as it is.  cam_out (nimages x 12 floats; may be cam itself), points_out (max_tracks x 4
        floats; may be points itself), cam_obs and cam_status (nimages ints: the observations used; 0 adjusted, 1 fewer
        than min_obs, 3 root or held, 4 no camera), cam_rms (nimages x 2 floats: rms reprojection error in px before and
        after), point_obs (max_tracks ints), history (num_loops x 4 words: the trial cost, the damping, kept, CG
        iterations), cost (2 floats: before, after) and summary (8 ints) are device buffers, allocated here when not
        passed; returns the nine.  Enqueued on the context stream."""
        return self._adjust_bundle("misift_adjust_bundle_batch", max_tracks, max_obs, track_offsets, obs, export_summary,
                                   points, point_status, nimages, cam, cam_pair, intrinsics, hold,
                                   (min_views, min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise), (),
                                   (cam_out, points_out, cam_obs, cam_status, cam_rms, point_obs, history, cost, summary))

    def _adjust_bundle(self, name, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                       nimages, cam, cam_pair, intrinsics, hold, steps, model, nine, obs_weight=_NO_ARGUMENT, more=()):
        """The body of the four adjust_bundle*_batch methods: the C function `name` on the scene, the hold list and
        steps (min_views ... orthonormalise), then `model` (what the call takes between orthonormalise and cam_out, as
        ctypes arguments), the nine outputs, obs_weight between cost and summary where the call has it (True allocates
        it, None or False leaves it out) and `more`, the outputs behind summary as (buffer or None, bytes).  An output
        that is None is allocated here; returns all of them in the order of the C call."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        hold = np.ascontiguousarray(hold, np.int32).reshape(-1)
        min_views, min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise = steps
        per_image, per_track = 4 * max(nimages, 1), 4 * max(max_tracks, 1)
        sizes = (12 * per_image, 4 * per_track, per_image, per_image, 2 * per_image, per_track,
                 16 * max(int(num_loops), 1), 8, 4 * 8)
        outs = [self.zeros(n) if b is None else b for b, n in zip(nine, sizes)]
        if obs_weight is not _NO_ARGUMENT:
            if obs_weight is True:
                obs_weight = self.zeros(4 * max(max_obs, 1))
            elif obs_weight is False:
                obs_weight = None
            outs.insert(8, obs_weight)
        outs += [self.zeros(n) if b is None else b for b, n in more]
        check(getattr(lib(), name)(
            self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs), _dptr(export_summary), _dptr(points),
            _dptr(point_status), nimages, _dptr(cam), _dptr(cam_pair), intrinsics.ctypes.data, len(hold),
            hold.ctypes.data if len(hold) else None, int(min_views), int(min_obs), int(num_loops), int(cg_iters),
            float(max_error), float(lambda0), int(orthonormalise), *model,
            *[_dptr(b) if b is not None else None for b in outs]), name)
        return tuple(outs)

    def adjust_bundle_robust_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                                   nimages, cam, cam_pair, intrinsics, hold=(), min_views=2, min_obs=6, num_loops=5,
                                   cg_iters=10, max_error=np.inf, lambda0=1e-3, orthonormalise=True, loss=LOSS_HUBER,
                                   loss_scale=2.0, cam_out=None, points_out=None, cam_obs=None, cam_status=None,
                                   cam_rms=None, point_obs=None, history=None, cost=None, obs_weight=True, summary=None):
        """misift_adjust_bundle_robust_batch: adjust_bundle_batch under a robust loss (LOSS_NONE, LOSS_HUBER,
        LOSS_GEMAN_MCCLURE) of scale loss_scale px: an observation far off its point is weighed down afresh in every
        step instead of pulling with its full square.  The arguments and the nine outputs are those of
        adjust_bundle_batch, where cam_rms, points_out[4t+3], history and cost now speak of the loss, not of the squared
        error; obs_weight (max_obs floats: the weight of each observation used under the final state, -1 for one not
        used) is a device buffer, allocated here when True, left out when None or False; returns the ten (obs_weight
        None when left out).  Enqueued on the context stream."""
        return self._adjust_bundle("misift_adjust_bundle_robust_batch", max_tracks, max_obs, track_offsets, obs,
                                   export_summary, points, point_status, nimages, cam, cam_pair, intrinsics, hold,
                                   (min_views, min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise),
                                   (int(loss), float(loss_scale)),
                                   (cam_out, points_out, cam_obs, cam_status, cam_rms, point_obs, history, cost, summary),
                                   obs_weight)

    def adjust_bundle_focal_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                                  nimages, cam, cam_pair, intrinsics, group, ngroups=None, hold=(), min_views=2,
                                  min_obs=6, num_loops=5, cg_iters=10, max_error=np.inf, lambda0=1e-3,
                                  orthonormalise=True, loss=LOSS_NONE, loss_scale=2.0, cam_out=None, points_out=None,
                                  cam_obs=None, cam_status=None, cam_rms=None, point_obs=None, history=None, cost=None,
                                  obs_weight=None, summary=None, intrinsics_out=None, focal=None):
        """misift_adjust_bundle_focal_batch: adjust_bundle_robust_batch with one focal scale per physical camera among
        the unknowns.  group (host, nimages ints) names the camera that took each image, -1 for an image whose
        intrinsics stay as given; ngroups (at most MAX_FOCAL_GROUPS) defaults to max(group) + 1.  The further arguments
        and the ten outputs are those of adjust_bundle_robust_batch (obs_weight: None or False leaves it out, True
        allocates it); intrinsics_out (nimages x 4 floats: fx*s, fy*s, cx, cy under the final scales, to be read back
        and handed to the next call of the chain) and focal (ngroups x 3 words: the scale, the members, FOCAL_*) are
        device buffers, allocated here when not passed; returns the twelve.  Enqueued on the context stream."""
        group = np.ascontiguousarray(group, np.int32).reshape(-1)
        if ngroups is None:
            ngroups = int(group.max()) + 1 if len(group) else 0
        assert ngroups == 0 or len(group) == nimages
        return self._adjust_bundle("misift_adjust_bundle_focal_batch", max_tracks, max_obs, track_offsets, obs,
                                   export_summary, points, point_status, nimages, cam, cam_pair, intrinsics, hold,
                                   (min_views, min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise),
                                   (int(loss), float(loss_scale), int(ngroups), group.ctypes.data if len(group) else None),
                                   (cam_out, points_out, cam_obs, cam_status, cam_rms, point_obs, history, cost, summary),
                                   obs_weight, ((intrinsics_out, 16 * max(nimages, 1)), (focal, 12 * max(int(ngroups), 1))))

    def adjust_bundle_radial_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                                   nimages, cam, cam_pair, intrinsics, group, ngroups=None, radial=None, k0=None, hold=(),
                                   min_views=2, min_obs=6, num_loops=5, cg_iters=10, max_error=np.inf, lambda0=1e-3,
                                   orthonormalise=True, loss=LOSS_NONE, loss_scale=2.0, cam_out=None, points_out=None,
                                   cam_obs=None, cam_status=None, cam_rms=None, point_obs=None, history=None, cost=None,
                                   obs_weight=None, summary=None, intrinsics_out=None, focal=None, radial_out=None):
        """misift_adjust_bundle_radial_batch: adjust_bundle_focal_batch with one radial coefficient per camera group
        among the unknowns, applied to the observation (the model is in include/misift.h).  radial (host, ngroups ints,
        1 = the coefficient is an unknown) and k0 (host, ngroups floats, its start and, where radial is 0, held value)
        are both given or both None (all zero).  The further arguments and the twelve outputs are those of
        adjust_bundle_focal_batch; radial_out (ngroups x 3 words: the coefficient, the members, RADIAL_*) is a device
        buffer, allocated here when not passed, and what undistort_obs_batch takes; returns the thirteen.  Enqueued on
        the context stream."""
        group = np.ascontiguousarray(group, np.int32).reshape(-1)
        if ngroups is None:
            ngroups = int(group.max()) + 1 if len(group) else 0
        assert ngroups == 0 or len(group) == nimages
        assert (radial is None) == (k0 is None)
        if radial is not None:
            radial = np.ascontiguousarray(radial, np.int32).reshape(-1)
            k0 = np.ascontiguousarray(k0, np.float32).reshape(-1)
            assert len(radial) == ngroups and len(k0) == ngroups
        return self._adjust_bundle("misift_adjust_bundle_radial_batch", max_tracks, max_obs, track_offsets, obs,
                                   export_summary, points, point_status, nimages, cam, cam_pair, intrinsics, hold,
                                   (min_views, min_obs, num_loops, cg_iters, max_error, lambda0, orthonormalise),
                                   (int(loss), float(loss_scale), int(ngroups), group.ctypes.data if len(group) else None,
                                    radial.ctypes.data if radial is not None and len(radial) else None,
                                    k0.ctypes.data if k0 is not None and len(k0) else None),
                                   (cam_out, points_out, cam_obs, cam_status, cam_rms, point_obs, history, cost, summary),
                                   obs_weight, ((intrinsics_out, 16 * max(nimages, 1)), (focal, 12 * max(int(ngroups), 1)),
                                                (radial_out, 12 * max(int(ngroups), 1))))

    def undistort_obs_batch(self, max_obs, obs, export_summary, nimages, intrinsics, group, radial, ngroups=None,
                            obs_out=None):
        """misift_undistort_obs_batch: the observation list under the radial model with the coefficients of `radial`
        (the device buffer adjust_bundle_radial_batch wrote).  intrinsics are the given ones (host); obs_out may be obs
        itself and is allocated here when not passed; returns it.  Enqueued on the context stream."""
        group = np.ascontiguousarray(group, np.int32).reshape(-1)
        if ngroups is None:
            ngroups = int(group.max()) + 1 if len(group) else 0
        assert ngroups == 0 or len(group) == nimages
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        if obs_out is None:
            obs_out = self.zeros(16 * max(max_obs, 1))
        check(lib().misift_undistort_obs_batch(
            self.h, max_obs, _dptr(obs), _dptr(export_summary), nimages, intrinsics.ctypes.data, int(ngroups),
            group.ctypes.data if len(group) else None, _dptr(radial) if radial is not None else None, _dptr(obs_out)),
            "misift_undistort_obs_batch")
        return obs_out

    def filter_tracks_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                            nimages, cam, cam_pair, intrinsics, max_error=np.inf, max_cos=np.inf, min_angle_deg=None,
                            min_views=2, unique_frames=True, track_offsets_out=None, obs_out=None,
                            export_summary_out=None, points_out=None, point_views_out=None, point_status_out=None,
                            track_map=None, obs_map=True, summary=None):
        """misift_filter_tracks_batch: the observation lists (track_offsets, obs, export_summary: the outputs of
        export_tracks_batch for max_tracks and max_obs, or of an earlier call of this one) gated against the points
        (points, point_status) and the cameras (cam, cam_pair, for nimages images; intrinsics: host, nimages x 4) and
        written out again in export's format.  A view is dropped when its point is bad or behind its camera or its
        reprojection error reaches max_error px; with unique_frames, of several views of one frame only the one with the
        smallest error stays; a track is dropped when fewer than min_views views stay or when no two of their rays are
        further apart than the angle whose cosine is max_cos (min_angle_deg gives it in degrees instead; +inf: no
        test).  track_offsets_out, obs_out, export_summary_out, points_out (the points copied, the rms of the kept views
        in the fourth word), point_views_out, point_status_out go to triangulate, refine, resect and adjust as they are;
        track_map (max_tracks ints: the new number or the reason), obs_map (max_obs ints: the new slot or the reason;
        True allocates it, None leaves it out) and summary (8 ints) tell what became of what.  All are device buffers,
        allocated here when not passed; returns the nine.  Nothing may overlap.  Enqueued on the context stream."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        if min_angle_deg is not None:
            max_cos = float(np.float32(np.cos(np.deg2rad(min_angle_deg))))
        mt, mo = max(max_tracks, 1), max(max_obs, 1)
        if track_offsets_out is None:
            track_offsets_out = self.zeros(4 * (mt + 1))
        if obs_out is None:
            obs_out = self.zeros(16 * mo)
        if export_summary_out is None:
            export_summary_out = self.zeros(4 * 8)
        if points_out is None:
            points_out = self.zeros(16 * mt)
        if point_views_out is None:
            point_views_out = self.zeros(4 * mt)
        if point_status_out is None:
            point_status_out = self.zeros(4 * mt)
        if track_map is None:
            track_map = self.zeros(4 * mt)
        if obs_map is True:
            obs_map = self.zeros(4 * mo)
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_filter_tracks_batch(self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs),
                                               _dptr(export_summary), _dptr(points), _dptr(point_status), nimages,
                                               _dptr(cam), _dptr(cam_pair), intrinsics.ctypes.data, float(max_error),
                                               float(max_cos), int(min_views), int(unique_frames),
                                               _dptr(track_offsets_out), _dptr(obs_out), _dptr(export_summary_out),
                                               _dptr(points_out), _dptr(point_views_out), _dptr(point_status_out),
                                               _dptr(track_map), _dptr(obs_map), _dptr(summary)),
              "misift_filter_tracks_batch")
        return (track_offsets_out, obs_out, export_summary_out, points_out, point_views_out, point_status_out,
                track_map, obs_map, summary)

    def resect_cameras_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status,
                             nimages, intrinsics, images, seeds, max_cand, num_loops=1024, thresh=4.0, min_inliers=12,
                             only_unset=False, install=False, cam=None, cam_pair=None, res_cam=None, res_cand=None,
                             res_inliers=None, res_status=None, summary=None):
        """misift_resect_cameras_batch: the camera of each image in `images` (host, distinct indices; seeds: host, one
        rand() seed per entry) estimated from the observations its image makes (track_offsets, obs, export_summary: the
        outputs of export_tracks_batch for max_tracks and max_obs) of the points of triangulate_tracks_batch (points,
        point_status), by RANSAC over num_loops calibrated six-point solves; a candidate is an inlier when its point is
        in front and within thresh px.  intrinsics: host, nimages x 4 (fx fy cx cy).  An image with more than max_cand
        candidates is not searched.  With only_unset, an image whose cam_pair entry is not -2 is skipped; with install,
        a camera found goes into cam (nimages x 12) and cam_pair (CAM_RESECTED).  res_cam (nsel x 12 floats), res_cand,
        res_inliers and res_status (nsel ints: the candidates, the inliers of the picked hypothesis; 0 ok, 1 too few
        candidates, 2 fewer than min_inliers inliers, 3 skipped, 4 more than max_cand candidates) and summary (8 ints)
        are device buffers, allocated here when not passed; returns the five.  Enqueued on the context stream."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        images = np.ascontiguousarray(images, np.int32).reshape(-1)
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        nsel = len(images)
        assert len(seeds) == nsel
        if res_cam is None:
            res_cam = self.zeros(48 * max(nsel, 1))
        if res_cand is None:
            res_cand = self.zeros(4 * max(nsel, 1))
        if res_inliers is None:
            res_inliers = self.zeros(4 * max(nsel, 1))
        if res_status is None:
            res_status = self.zeros(4 * max(nsel, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_resect_cameras_batch(self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs),
                                                _dptr(export_summary), _dptr(points), _dptr(point_status), nimages,
                                                intrinsics.ctypes.data, nsel, images.ctypes.data if nsel else None,
                                                seeds.ctypes.data if nsel else None, int(max_cand), int(num_loops),
                                                float(thresh), int(min_inliers), int(only_unset), int(install),
                                                _dptr(cam), _dptr(cam_pair), _dptr(res_cam), _dptr(res_cand),
                                                _dptr(res_inliers), _dptr(res_status), _dptr(summary)),
              "misift_resect_cameras_batch")
        return res_cam, res_cand, res_inliers, res_status, summary

    def describe_points_batch(self, max_tracks, max_obs, track_offsets, obs, export_summary, points, point_status, q,
                              nframes, counts, offsets=None, stride=0, max_records=None, scene_q=None, scene_recs=None,
                              scene_count=None, point_members=None, summary=None):
        """misift_describe_points_batch: an 8-bit descriptor per track point (the rounded mean of the rows of q its
        observations name; q: quantize_batch's output for the record batch of nframes frames, counts, offsets or
        stride, max_records records) as a one-frame record set: scene_q (max_tracks x 128 bytes), scene_recs (max_tracks
        records whose xpos, ypos, scale are X, Y, Z), scene_count (1 int, T), point_members (max_tracks ints) and
        summary (8 ints: T, described points, their observations, observations that do not contribute) are device
        buffers, allocated here when None; returns the five.  match_pairs_batch_i8 takes them as recs2 = scene_recs,
        q2 = scene_q, nframes2 = 1, counts2 = scene_count, stride2 = max_tracks.  Enqueued on the context stream."""
        if scene_q is None:
            scene_q = self.zeros(128 * max_tracks)
        if scene_recs is None:
            scene_recs = self.zeros(POINT_DTYPE.itemsize * max_tracks)
        if scene_count is None:
            scene_count = self.zeros(4)
        if point_members is None:
            point_members = self.zeros(4 * max_tracks)
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_describe_points_batch(self.h, max_tracks, max_obs, _dptr(track_offsets), _dptr(obs),
                                                 _dptr(export_summary), _dptr(points), _dptr(point_status), _dptr(q),
                                                 nframes, _dptr(counts), _dptr(offsets), stride, int(max_records),
                                                 _dptr(scene_q), _dptr(scene_recs), _dptr(scene_count),
                                                 _dptr(point_members), _dptr(summary)),
              "misift_describe_points_batch")
        return scene_q, scene_recs, scene_count, point_members, summary

    def localize_frames_batch(self, rows, nframes_rows, counts, offsets, stride, max_tracks, export_summary, points,
                              point_status, nimages, intrinsics, frames, images, seeds, max_pts, max_found,
                              min_score=0.85, max_ambiguity=0.95, num_loops=1024, thresh=4.0, min_inliers=12,
                              only_unset=False, install=False, cam=None, cam_pair=None, res_cam=None, res_cand=None,
                              res_inliers=None, res_status=None, summary=None, found_offsets=None, found_obs=None,
                              found_summary=None, found_points=None, found_views=None, found_status=None,
                              found_map=None):
        """misift_localize_frames_batch: the camera of image images[e] from the rows of frame frames[e] (rows: a batch of
        nframes_rows frames, counts, offsets or stride, as find_homography_batch takes it; after match_pairs_batch_i8
        against describe_points_batch's scene: frame = pair, stride = max_pts, counts = out_counts) whose match names
        a point of the scene (export_summary, points, point_status for max_tracks), by resect_cameras_batch's search
        over the rows that pass min_score and max_ambiguity; seeds, num_loops, thresh, min_inliers, only_unset, install,
        cam, cam_pair and the five res_* / summary outputs as in resect_cameras_batch (status 4: more than max_pts
        rows).  The inliers go out as a scene for merge_scenes_batch: found_offsets (max_found + 1 ints), found_obs
        (max_found observations), found_summary (8 ints, export's layout), found_points (max_found x 4 floats),
        found_views, found_status and found_map (max_found ints each: the point of the scene each find belongs to, the
        merge's point_map).  Device buffers are allocated here when None; returns a dict of the twelve outputs.
        Enqueued on the context stream."""
        intrinsics = np.ascontiguousarray(intrinsics, np.float32).reshape(-1, 4)
        assert len(intrinsics) == nimages
        frames = np.ascontiguousarray(frames, np.int32).reshape(-1)
        images = np.ascontiguousarray(images, np.int32).reshape(-1)
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        nsel = len(frames)
        assert len(images) == nsel and len(seeds) == nsel
        n, m = max(nsel, 1), max(max_found, 1)
        sizes = dict(res_cam=48 * n, res_cand=4 * n, res_inliers=4 * n, res_status=4 * n, summary=32,
                     found_offsets=4 * (m + 1), found_obs=16 * m, found_summary=32, found_points=16 * m,
                     found_views=4 * m, found_status=4 * m, found_map=4 * m)
        given = dict(res_cam=res_cam, res_cand=res_cand, res_inliers=res_inliers, res_status=res_status, summary=summary,
                     found_offsets=found_offsets, found_obs=found_obs, found_summary=found_summary,
                     found_points=found_points, found_views=found_views, found_status=found_status, found_map=found_map)
        o = {k: self.zeros(sizes[k]) if v is None else v for k, v in given.items()}
        check(lib().misift_localize_frames_batch(
            self.h, _dptr(rows), nframes_rows, _dptr(counts), _dptr(offsets), stride, max_tracks, _dptr(export_summary),
            _dptr(points), _dptr(point_status), nimages, intrinsics.ctypes.data, nsel,
            frames.ctypes.data if nsel else None, images.ctypes.data if nsel else None,
            seeds.ctypes.data if nsel else None, int(max_pts), float(min_score), float(max_ambiguity), int(num_loops),
            float(thresh), int(min_inliers), int(only_unset), int(install), _dptr(cam), _dptr(cam_pair),
            _dptr(o["res_cam"]), _dptr(o["res_cand"]), _dptr(o["res_inliers"]), _dptr(o["res_status"]),
            _dptr(o["summary"]), int(max_found), _dptr(o["found_offsets"]), _dptr(o["found_obs"]),
            _dptr(o["found_summary"]), _dptr(o["found_points"]), _dptr(o["found_views"]), _dptr(o["found_status"]),
            _dptr(o["found_map"])), "misift_localize_frames_batch")
        return o

    def correspond_tracks_batch(self, max_records_a, record_obs_a, max_tracks_a, max_obs_a, track_offsets_a,
                                export_summary_a, max_records_b, record_obs_b, max_tracks_b, max_obs_b, track_offsets_b,
                                export_summary_b, shift=0, track_map=None, summary=None):
        """misift_correspond_tracks_batch: for every track of exported scene A the track of scene B that holds the same
        records (record g of A is record g - shift of B), -1 for none and -2 for several.  record_obs_*: the
        d_record_obs of export_tracks_batch, filled with -1 before the export.  track_map (max_tracks_a ints) and
        summary (8 ints: T_A, T_B, ties, mapped, in conflict) are device buffers, allocated here when not passed;
        returns the two.  Enqueued on the context stream."""
        if track_map is None:
            track_map = self.zeros(4 * max_tracks_a)
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_correspond_tracks_batch(self.h, int(shift), max_records_a, _dptr(record_obs_a), max_tracks_a,
                                                   max_obs_a, _dptr(track_offsets_a), _dptr(export_summary_a),
                                                   max_records_b, _dptr(record_obs_b), max_tracks_b, max_obs_b,
                                                   _dptr(track_offsets_b), _dptr(export_summary_b), _dptr(track_map),
                                                   _dptr(summary)), "misift_correspond_tracks_batch")
        return track_map, summary

    def align_points_batch(self, src, dst, point_map, ranges, seeds, src_status=None, dst_status=None, count=None,
                           count_stride=1, num_loops=256, thresh=0.05, min_inliers=3, refit_loops=5, sim=None,
                           align_cand=None, align_inliers=None, align_status=None, inlier=None, summary=None):
        """misift_align_points_batch: per entry the similarity transform b = s R a + t between the points of src and
        their correspondents in dst (pooled device arrays of 4 floats per point; point_map: per source point the index
        of its correspondent relative to the entry's dst_first, or negative), by RANSAC over num_loops three-point
        solves with the 3-D distance thresh, refitted refit_loops times over its inliers.  ranges: host, nsel x 4
        (src_first, src_cap, dst_first, dst_cap); seeds: host, one rand() seed per entry; count: device, the number of
        source points of entry e at count[e * count_stride], or None for src_cap.  sim (nsel x 16 floats: R, t, s, rms),
        align_cand, align_inliers, align_status (nsel ints; 0 ok, 1 too few candidates, 2 fewer than min_inliers
        inliers) and summary (8 ints) are device buffers, allocated here when not passed; inlier (one int per source
        point) is written only when passed.  Returns the five.  Enqueued on the context stream."""
        ranges = np.ascontiguousarray(ranges, np.int32).reshape(-1, 4)
        seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        nsel = len(ranges)
        assert len(seeds) == nsel
        if sim is None:
            sim = self.zeros(64 * max(nsel, 1))
        if align_cand is None:
            align_cand = self.zeros(4 * max(nsel, 1))
        if align_inliers is None:
            align_inliers = self.zeros(4 * max(nsel, 1))
        if align_status is None:
            align_status = self.zeros(4 * max(nsel, 1))
        if summary is None:
            summary = self.zeros(4 * 8)
        check(lib().misift_align_points_batch(self.h, _dptr(src), _dptr(src_status), _dptr(dst), _dptr(dst_status),
                                              _dptr(point_map), nsel, ranges.ctypes.data if nsel else None,
                                              seeds.ctypes.data if nsel else None, _dptr(count), int(count_stride),
                                              int(num_loops), float(thresh), int(min_inliers), int(refit_loops),
                                              _dptr(sim), _dptr(align_cand), _dptr(align_inliers), _dptr(align_status),
                                              _dptr(inlier), _dptr(summary)), "misift_align_points_batch")
        return sim, align_cand, align_inliers, align_status, summary

    def transform_scene_batch(self, sim, max_tracks, export_summary, points, point_status, nimages, cam, cam_pair,
                              sim_status=None, points_out=None, cam_out=None):
        """misift_transform_scene_batch: the transform sim (16 device floats, one entry of align_points_batch; applied
        only when sim_status, its device status word, is None or holds 0) applied to the points with status 0 of the
        first T tracks and to the cameras that are set, so that every reprojection is unchanged; everything else is
        copied.  points_out and cam_out may be points and cam; allocated here when not passed.  Returns the two."""
        if points_out is None:
            points_out = self.zeros(16 * max_tracks)
        if cam_out is None:
            cam_out = self.zeros(48 * nimages)
        check(lib().misift_transform_scene_batch(self.h, _dptr(sim), _dptr(sim_status), max_tracks,
                                                 _dptr(export_summary), _dptr(points), _dptr(point_status), nimages,
                                                 _dptr(cam), _dptr(cam_pair), _dptr(points_out), _dptr(cam_out)),
              "misift_transform_scene_batch")
        return points_out, cam_out

    def merge_scenes_batch(self, a, b, point_map, nimages_out, max_tracks_out, max_obs_out, accept=None, fshift_a=0,
                           fshift_b=0, rshift_a=0, rshift_b=0, max_records_out=0, track_offsets_out=None, obs_out=None,
                           export_summary_out=None, points_out=None, point_views_out=None, point_status_out=None,
                           cam_out=None, cam_pair_out=None, track_map_a=None, obs_map_a=True, obs_map_b=True,
                           record_obs_out=None, summary=None):
        """misift_merge_scenes_batch: scene a (after transform_scene_batch has moved it into b's gauge) and scene b
        written out as one scene in export's format.  a and b are dicts of the MERGE_SCENE_KEYS: the capacities and
        device buffers of export_tracks_batch (track_offsets, obs, export_summary, and record_obs with max_records when
        record_obs_out is wanted), of triangulate_tracks_batch (points, point_views, point_status) and the cameras
        (nimages, cam, cam_pair).  point_map: the track_map of correspond_tracks_batch(a, b); accept: the inlier buffer
        of align_points_batch over a's tracks, or None.  Image i of a is image i + fshift_a of the merged scene of
        nimages_out images, record g of a is record g + rshift_a of max_records_out, and likewise for b.  b's tracks
        keep their numbers and a's unmatched tracks follow; an observation both scenes hold stays once, as b's.
        track_offsets_out, obs_out, export_summary_out, points_out, point_views_out, point_status_out, cam_out and
        cam_pair_out go to triangulate, refine, resect, filter and adjust as they are; track_map_a (a's max_tracks
        ints), obs_map_a, obs_map_b (True allocates, None leaves out), record_obs_out (True allocates; needs both
        record_obs) and summary (8 ints) tell what became of what.  All are device buffers, allocated here when not
        passed; returns a dict of the MERGE_OUTPUTS.  Nothing may overlap.  Enqueued on the context stream."""
        mt, mo, ni = max(max_tracks_out, 1), max(max_obs_out, 1), max(nimages_out, 1)
        outs = dict(track_offsets_out=track_offsets_out, obs_out=obs_out, export_summary_out=export_summary_out,
                    points_out=points_out, point_views_out=point_views_out, point_status_out=point_status_out,
                    cam_out=cam_out, cam_pair_out=cam_pair_out, track_map_a=track_map_a, obs_map_a=obs_map_a,
                    obs_map_b=obs_map_b, record_obs_out=record_obs_out, summary=summary)
        sizes = dict(track_offsets_out=4 * (mt + 1), obs_out=16 * mo, export_summary_out=32, points_out=16 * mt,
                     point_views_out=4 * mt, point_status_out=4 * mt, cam_out=48 * ni, cam_pair_out=4 * ni,
                     track_map_a=4 * max(a["max_tracks"], 1), obs_map_a=4 * max(a["max_obs"], 1),
                     obs_map_b=4 * max(b["max_obs"], 1), record_obs_out=4 * max(max_records_out, 1), summary=32)
        optional = ("obs_map_a", "obs_map_b", "record_obs_out")
        for k in MERGE_OUTPUTS:
            if outs[k] is True or (outs[k] is None and k not in optional):
                outs[k] = self.zeros(sizes[k])

        def scene(s):
            return [_dptr(s.get(k)) if k in ("track_offsets", "obs", "export_summary", "points", "point_views",
                                             "point_status", "cam", "cam_pair", "record_obs") else int(s.get(k) or 0)
                    for k in MERGE_SCENE_KEYS]

        check(lib().misift_merge_scenes_batch(self.h, *scene(a), *scene(b), _dptr(point_map), _dptr(accept),
                                              int(fshift_a), int(fshift_b), int(nimages_out), int(rshift_a),
                                              int(rshift_b), int(max_records_out), int(max_tracks_out),
                                              int(max_obs_out), *[_dptr(outs[k]) for k in MERGE_OUTPUTS]),
              "misift_merge_scenes_batch")
        return outs

    merge_scenes = merge_scenes_batch

    def match_split(self, pts1, n1, pts2, n2, own_tile_begin, own_tile_end):
        """Test hook: misift_match with the column sweep cut into two launches (the sharded matcher's cut)."""
        d1 = self.upload(pts1)
        d2 = self.upload(pts2)
        check(lib().misift_test_match_split(self.h, d1.ptr, n1, d2.ptr, n2, own_tile_begin, own_tile_end),
              "misift_test_match_split")
        return self.download(d1, (len(pts1),), POINT_DTYPE)

    def find_homography(self, dpts_ptr, npts, num_loops=1000, min_score=0.85, max_ambiguity=0.95, thresh=5.0):
        H = (C.c_float * 9)()
        nm = C.c_int(0)
        check(lib().misift_find_homography(self.h, dpts_ptr, npts, H, C.byref(nm), num_loops, min_score,
                                           max_ambiguity, thresh), "misift_find_homography")
        return np.array(list(H), np.float32).reshape(3, 3), nm.value

    def improve_homography(self, dpts_ptr, npts, H, num_loops=5, min_score=0.0, max_ambiguity=0.80, thresh=3.0):
        h = (C.c_float * 9)(*[float(v) for v in np.asarray(H, np.float32).reshape(9)])
        nf = C.c_int(0)
        check(lib().misift_improve_homography(self.h, dpts_ptr, npts, h, num_loops, min_score, max_ambiguity, thresh,
                                              C.byref(nf)), "misift_improve_homography")
        return np.array(list(h), np.float32).reshape(3, 3), nf.value

    def test_elementary(self, fn, x, y=None):
        """Device copies of det_exp2 (0) / det_atan2(y, x) (1) / det_exp (2) / det_sincos (3) on float32 arrays."""
        x = np.ascontiguousarray(x, np.float32)
        dx = self.upload(x)
        dy = self.upload(np.ascontiguousarray(y, np.float32)) if y is not None else None
        o1, o2 = self.zeros(4 * len(x)), self.zeros(4 * len(x))
        check(lib().misift_test_elementary(self.h, fn, dx.ptr, dy.ptr if dy else None, o1.ptr, o2.ptr, len(x)),
              "misift_test_elementary")
        a = self.download(o1, (len(x),), np.float32)
        return (a, self.download(o2, (len(x),), np.float32)) if fn == 3 else a

    # ---- profiling
    def profile_enable(self, on=True):
        check(lib().misift_profile_enable(self.h, int(on)), "misift_profile_enable")

    def profile_reset(self):
        check(lib().misift_profile_reset(self.h), "misift_profile_reset")

    def profile_read(self):
        cap = 32
        names = C.create_string_buffer(32 * cap)
        ms = (C.c_float * cap)()
        calls = (C.c_int * cap)()
        n = C.c_int(0)
        check(lib().misift_profile_read(self.h, cap, C.cast(names, C.c_void_p), ms, calls, C.byref(n)),
              "misift_profile_read")
        out = {}
        for i in range(n.value):
            nm = names.raw[32 * i:32 * i + 32].split(b"\0")[0].decode()
            out[nm] = {"total_ms": float(ms[i]), "calls": int(calls[i])}
        return out


class HipEvent:
    """A raw hipEvent_t (timing enabled) for the entry points that take one as void*: misift_ctx_record_batch."""
    _hip = None

    def __init__(self):
        if HipEvent._hip is None:
            HipEvent._hip = hip_runtime()
            HipEvent._hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            HipEvent._hip.hipStreamWaitEvent.argtypes = [C.c_void_p, C.c_void_p, C.c_uint]
            HipEvent._hip.hipEventSynchronize.argtypes = [C.c_void_p]
            HipEvent._hip.hipEventDestroy.argtypes = [C.c_void_p]
        self.h = C.c_void_p()
        if HipEvent._hip.hipEventCreate(C.byref(self.h)) != 0:
            raise MisiftError("hipEventCreate failed")

    def synchronize(self):
        if HipEvent._hip.hipEventSynchronize(self.h) != 0:
            raise MisiftError("hipEventSynchronize failed")

    def stream_wait(self, stream):
        """`stream` (raw hipStream_t value) waits for this event."""
        if HipEvent._hip.hipStreamWaitEvent(C.c_void_p(stream), self.h, 0) != 0:
            raise MisiftError("hipStreamWaitEvent failed")

    def elapsed_time(self, later):
        ms = C.c_float(0)
        if HipEvent._hip.hipEventElapsedTime(C.byref(ms), self.h, later.h) != 0:
            raise MisiftError("hipEventElapsedTime failed")
        return ms.value

    def __del__(self):
        try:
            if self.h:
                HipEvent._hip.hipEventDestroy(self.h)
                self.h = None
        except Exception:
            pass


COMM_ID_BYTES = 128
RESULT_DTYPE = np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4")])      # 12 B/row (misift_match_sharded)
# the 528-byte match column misift_match_sharded ships and leaves in d_set2_all (MISIFT_MATCH_COLUMN_BYTES)
COLUMN_DTYPE = np.dtype([("data", "<f4", (128,)), ("xpos", "<f4"), ("ypos", "<f4"), ("reserved", "<f4", (2,))])
assert COLUMN_DTYPE.itemsize == 528


def comm_unique_id():
    """128 opaque bytes made by rank 0 (ncclGetUniqueId); ship them to the other ranks, then Comm(ctx, n, r, id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(lib().misift_comm_unique_id(C.cast(buf, C.c_void_p)), "misift_comm_unique_id")
    return buf.raw


class LoopbackWorld:
    """misift_loopback_world: the rendezvous object of N in-process communicators (fake N ranks on one GPU)."""

    def __init__(self, nranks):
        h = C.c_void_p()
        check(lib().misift_loopback_world_create(nranks, C.byref(h)), "misift_loopback_world_create")
        self.h, self.size = h, nranks

    def close(self):
        if self.h:
            lib().misift_loopback_world_destroy(self.h)
            self.h = None


class Comm:
    """One communicator per context (misift_comm_*): the multi-GPU entry points of the C-ABI.
    id_bytes: the 128-byte RCCL id — or a LoopbackWorld for the in-process transport."""

    def __init__(self, ctx, nranks, rank, id_bytes):
        h = C.c_void_p()
        if isinstance(id_bytes, LoopbackWorld):
            assert nranks == id_bytes.size
            check(lib().misift_comm_create_loopback(ctx.h, id_bytes.h, rank, C.byref(h)), "misift_comm_create_loopback")
        else:
            assert len(id_bytes) == COMM_ID_BYTES
            buf = C.create_string_buffer(bytes(id_bytes), COMM_ID_BYTES)
            check(lib().misift_comm_create(ctx.h, nranks, rank, C.cast(buf, C.c_void_p), C.byref(h)), "misift_comm_create")
        self.h = h
        self.ctx = ctx
        self.rank, self.size = lib().misift_comm_rank(h), lib().misift_comm_size(h)

    def barrier(self):
        check(lib().misift_comm_barrier(self.h), "misift_comm_barrier")

    def gather_post(self, slot, d_counts, nframes, d_packed, ctx=None):
        """ctx: the context (of the communicator's device) whose stream produced the buffers; default = the communicator's own."""
        check(lib().misift_gather_post((ctx or self.ctx).h, self.h, slot, d_counts, nframes, d_packed), "misift_gather_post")

    def gather_test(self, slot):
        """True once the batch posted in `slot` has finished on the GPU (non-blocking)."""
        r = C.c_int(0)
        check(lib().misift_gather_test(self.h, slot, C.byref(r)), "misift_gather_test")
        return bool(r.value)

    def gather_complete(self, slot, nframes, root=0, d_recv=None, capacity_records=0):
        """Returns (all_counts [size, nframes] int32, rank offsets [size+1] in records)."""
        counts = np.zeros((self.size, nframes), np.int32)
        offs = (C.c_size_t * (self.size + 1))()
        check(lib().misift_gather_complete(self.h, slot, root, counts.ctypes.data, d_recv, capacity_records, offs),
              "misift_gather_complete")
        return counts, np.array(list(offs), np.int64)

    def wire_bytes(self):
        """(received, sent) payload bytes of this rank since the communicator was created."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib().misift_comm_wire_bytes(self.h, C.byref(a), C.byref(b)), "misift_comm_wire_bytes")
        return int(a.value), int(b.value)

    def match_sharded(self, d_rows1, row_count, d_shard2, shard_count, d_set2_all, d_results_all=None):
        check(lib().misift_match_sharded(self.ctx.h, self.h, d_rows1, row_count, d_shard2, shard_count, d_set2_all,
                                         d_results_all), "misift_match_sharded")

    def close(self):
        if self.h:
            lib().misift_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _HostTransport(C.Structure):
    """misift_host_transport (include/misift.h)."""
    AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)
    P2P = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int)
    END = C.CFUNCTYPE(C.c_int, C.c_void_p)
    _fields_ = [("user", C.c_void_p), ("allgather", AG), ("send", P2P), ("recv", P2P), ("group_end", END)]


class HostComm(Comm):
    """A HOST communicator (misift_comm_create_host): no device; counts / packed records / receive buffers are host
    memory (numpy arrays), the exchange primitives are Python callables — tests/test_dist_cpu.py implements them with
    torch.distributed (gloo), so the gather logic of multigpu.hip itself runs on a machine without GPUs.

    allgather(send_ptr, recv_ptr, nbytes), send(ptr, nbytes, peer), recv(ptr, nbytes, peer), group_end(): raise on error."""

    def __init__(self, nranks, rank, allgather, send, recv, group_end):     # noqa: super().__init__ not called on purpose
        def guard(fn):
            def call(_user, *a):
                try:
                    fn(*a)
                    return 0
                except Exception:                    # noqa: BLE001 — reported through the C-ABI's error path
                    import traceback
                    traceback.print_exc()
                    return 1
            return call
        self._cb = _HostTransport(None, _HostTransport.AG(guard(allgather)), _HostTransport.P2P(guard(send)),
                                  _HostTransport.P2P(guard(recv)), _HostTransport.END(guard(group_end)))
        h = C.c_void_p()
        check(lib().misift_comm_create_host(nranks, rank, C.byref(self._cb), C.byref(h)), "misift_comm_create_host")
        self.h = h
        self.ctx = None
        self.rank, self.size = lib().misift_comm_rank(h), lib().misift_comm_size(h)

    def gather_post(self, slot, counts, nframes, packed, ctx=None):
        """counts: int32 numpy [nframes]; packed: uint8 numpy (both must stay alive until gather_complete)."""
        check(lib().misift_gather_post(None, self.h, slot, counts.ctypes.data, nframes, packed.ctypes.data), "misift_gather_post")

    def gather_complete(self, slot, nframes, root=0, recv=None, capacity_records=0):
        counts = np.zeros((self.size, nframes), np.int32)
        offs = (C.c_size_t * (self.size + 1))()
        check(lib().misift_gather_complete(self.h, slot, root, counts.ctypes.data, recv.ctypes.data if recv is not None else None,
                                           capacity_records, offs), "misift_gather_complete")
        return counts, np.array(list(offs), np.int64)


class PinnedArray:
    """numpy view over pinned host memory (misift_host_alloc) — uploads/downloads from it are asynchronous."""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(shape)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().misift_host_alloc(max(nbytes, 1), C.byref(p)), "misift_host_alloc")
        self.ptr = p.value
        buf = (C.c_char * nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().misift_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Pipe:
    """Host-fed extraction pipeline (misift_pipe_*): submit batches of host frames, collect packed records."""

    def __init__(self, ctx, width, height, batch_frames, src_u8=True, num_octaves=5, init_blur=1.0, thresh=3.0,
                 lowest_scale=0.0, max_pts=32768, depth=2):
        h = C.c_void_p()
        check(lib().misift_pipe_create(ctx.h, width, height, batch_frames, int(bool(src_u8)), num_octaves, init_blur,
                                       thresh, lowest_scale, max_pts, depth, C.byref(h)), "misift_pipe_create")
        self.h = h
        self.ctx = ctx
        self.batch = batch_frames
        self.max_pts = max_pts

    def submit(self, host_ptr, nframes):
        check(lib().misift_pipe_submit(self.h, host_ptr, nframes), "misift_pipe_submit")

    def collect(self, out_ptr=None, capacity_records=0):
        """Returns (counts[nframes], nrecords).  Records go to out_ptr (capacity in records) when given."""
        nf = C.c_int(0)
        cnt = (C.c_int * self.batch)()
        nrec = C.c_size_t(0)
        check(lib().misift_pipe_collect(self.h, C.byref(nf), cnt, out_ptr, capacity_records, C.byref(nrec)),
              "misift_pipe_collect")
        return np.array(list(cnt)[:nf.value], np.int32), int(nrec.value)

    def pending(self):
        return lib().misift_pipe_pending(self.h)

    def close(self):
        if self.h:
            lib().misift_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
