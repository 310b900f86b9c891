"""ctypes binding of liblvk_hip.so (the C ABI declared in include/lvk_c.h)."""
import ctypes as C
import weakref
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("LVK_LIB", os.path.join(_HERE, "liblvk_hip.so"))
_LIB = None

PT = np.dtype([("x", np.float32), ("y", np.float32)])
IMU = np.dtype([("t", np.float64), ("gyro", np.float64, 3), ("acc", np.float64, 3)])
OBS = np.dtype([("id", np.uint64), ("u", np.float64), ("v", np.float64), ("u_init", np.float64),
                ("v_init", np.float64), ("u_vel", np.float64), ("v_vel", np.float64),
                ("u_init_vel", np.float64), ("v_init_vel", np.float64)])

# every symbol include/lvk_c.h declares (checked by tests/test_abi.py against the header text)
ABI_SYMBOLS = [
    "lvk_runtime_env", "lvk_context_create", "lvk_context_destroy", "lvk_context_set_stream", "lvk_context_get_stream", "lvk_sync", "lvk_last_error", "lvk_version",
    "lvk_malloc", "lvk_free", "lvk_memcpy_h2d", "lvk_memcpy_d2h", "lvk_memset",
    "lvk_clahe_u8", "lvk_pyramid_create", "lvk_pyramid_destroy", "lvk_pyramid_build", "lvk_pyramid_build_clahe",
    "lvk_pyramid_levels", "lvk_pyramid_level", "lvk_orb_prepare", "lvk_image_to_gray", "lvk_min_eigen_map", "lvk_good_features", "lvk_good_features_from_map",
    "lvk_lk_track", "lvk_orb_describe", "lvk_hamming256_rows", "lvk_undistort_points", "lvk_find_fundamental_mask", "lvk_find_fundamental",
    "lvk_ransac_fundamental", "lvk_orb_match_guided", "lvk_align_ransac_2pt", "lvk_align_draw_pairs", "lvk_map_select_queries", "lvk_map_build", "lvk_orb_match_global", "lvk_align_ransac_3d", "lvk_align_invert", "lvk_map_transform", "lvk_predict_homography",
    "lvk_frontend_create", "lvk_frontend_destroy", "lvk_frontend_process", "lvk_frontend_tracks", "lvk_frontend_new_pts",
    "lvk_frontend_set_mask", "lvk_frontend_has_mask", "lvk_frontend_set_input_format", "lvk_frontend_input_format", "lvk_frontend_match_landmarks", "lvk_frontend_align_landmarks",
    "lvk_frontend_set_map", "lvk_frontend_map_size", "lvk_frontend_build_map", "lvk_frontend_match_map", "lvk_frontend_relocalise_map", "lvk_frontend_merge_map",
    "lvk_frontend_state", "lvk_frontend_lk_stats", "lvk_frontend_msg_stats", "lvk_frontend_profile_enable", "lvk_frontend_profile_read",
    "lvk_frontend_stage_name", "lvk_fe_track_stage", "lvk_fe_commit_stage", "lvk_fe_msg_stage",
    "lvk_ekf_compress_qr", "lvk_ekf_compress_qr_groups", "lvk_ekf_qr_plan", "lvk_ekf_update", "lvk_ekf_update_ldlt", "lvk_ekf_update_ldlt_perm", "lvk_dgemm", "lvk_dgemm_ex", "lvk_chol_solve", "lvk_ekf_cov_propagate_augment", "lvk_ekf_cov_gather", "lvk_ekf_cov_reanchor", "lvk_ekf_cov_append_features", "lvk_ekf_landmark_cov", "lvk_ekf_pose_rel_cov", "lvk_ekf_landmark_rel_cov", "lvk_ekf_msckf_point_cov", "lvk_ekf_update_sparse", "lvk_ekf_update_landmarks", "lvk_ekf_camera_pose_cov", "lvk_map_gather_obs", "lvk_vio_localise_map", "lvk_ekf_create", "lvk_ekf_destroy", "lvk_ekf_process", "lvk_ekf_process_async", "lvk_ekf_wait", "lvk_ekf_set_state",
    "lvk_ekf_dim", "lvk_ekf_is_initialized", "lvk_ekf_take_off_stamp", "lvk_ekf_get_state", "lvk_ekf_get_imu_intrinsics", "lvk_ekf_set_imu_intrinsics", "lvk_ekf_get_cov", "lvk_ekf_set_cov", "lvk_ekf_set_indefinite_policy", "lvk_ekf_indefinite_fallbacks", "lvk_ekf_last_update", "lvk_ekf_get_cov_imu", "lvk_ekf_get_clones", "lvk_ekf_get_features", "lvk_ekf_take_lost_features", "lvk_ekf_get_feature_cov", "lvk_ekf_set_lost_feature_cov", "lvk_ekf_take_lost_features_cov", "lvk_ekf_get_feature_rel", "lvk_ekf_set_msckf_points", "lvk_ekf_take_msckf_points", "lvk_ekf_set_keyframe_export", "lvk_ekf_take_keyframes", "lvk_ekf_get_window_cov", "lvk_ekf_add_fix", "lvk_ekf_set_fix_options", "lvk_ekf_take_fix_reports", "lvk_ekf_fix_stats", "lvk_ekf_add_landmark_obs", "lvk_ekf_set_landmark_options", "lvk_ekf_take_landmark_reports", "lvk_ekf_landmark_stats",
    "lvk_ekf_counters", "lvk_ekf_init_report", "lvk_ekf_profile", "lvk_ekf_profile_qr", "lvk_ekf_set_shard", "lvk_ekf_shard_stats", "lvk_shard_unique_id", "lvk_shard_comm_create", "lvk_shard_comm_destroy", "lvk_shard_comm_error", "lvk_shard_rccl_path", "lvk_shard_allgather_rccl", "lvk_shard_pack_stage", "lvk_shard_unpack_stage", "lvk_triangulate", "lvk_ekf_gate_and_stack", "lvk_ekf_feature_rows", "lvk_vio_process", "lvk_vio_process_deferred", "lvk_vio_pipe_create", "lvk_vio_pipe_destroy", "lvk_vio_pipe_push_imu", "lvk_vio_pipe_submit", "lvk_vio_pipe_drain", "lvk_vio_pipe_on_update", "lvk_vio_pipe_stats", "lvk_vio_pipe_latency", "lvk_vio_pipe_early_counts",
]
FE_STAGES = 9


class LvkError(RuntimeError):
    pass


class Image(C.Structure):
    """lvk_image: pointer + the size and step a cv::Mat carries (include/lvk_c.h)"""
    _fields_ = [("data", C.c_void_p), ("width", C.c_int), ("height", C.c_int), ("stride", C.c_int), ("is_device", C.c_int)]


# LVK_PIX_* of include/lvk_c.h by name, and what a host array of each format looks like: (dtype, trailing dimension or None, bytes per pixel)
PIX_FORMATS = {"mono8": 0, "bgr8": 1, "rgb8": 2, "bgra8": 3, "rgba8": 4, "mono16": 5, "yuyv": 6, "uyvy": 7}
_PIX_ARRAY = {"mono8": (np.uint8, None, 1), "bgr8": (np.uint8, 3, 3), "rgb8": (np.uint8, 3, 3), "bgra8": (np.uint8, 4, 4), "rgba8": (np.uint8, 4, 4),
              "mono16": (np.uint16, None, 2), "yuyv": (np.uint8, 2, 2), "uyvy": (np.uint8, 2, 2)}


def pixfmt_bytes_per_pixel(fmt):
    return _PIX_ARRAY[fmt][2]


def pixfmt_host_array(img, fmt):
    """The array an image of pixel format `fmt` must be: (H, W, 3|4) uint8 for the colour formats, (H, W) uint16 for mono16, (H, W, 2)
    uint8 for the two YUV 4:2:2 layouts.  Returns it with contiguous pixels (rows may be strided); anything else is a ValueError that
    names both the array and the format."""
    dtype, last, _ = _PIX_ARRAY[fmt]
    img = np.asarray(img)
    want = f"(H, W{'' if last is None else ', %d' % last}) {np.dtype(dtype).name}"
    if img.dtype != dtype or img.ndim != (2 if last is None else 3) or (last is not None and img.shape[2] != last):
        raise ValueError(f"a {img.dtype.name} array of shape {img.shape} is not a {fmt} image: {want} is expected")
    ok = img.strides[1] == img.itemsize * (last or 1) and (last is None or img.strides[2] == 1) and img.strides[0] >= img.shape[1] * img.strides[1]
    return img if ok else np.ascontiguousarray(img)


def make_image(img=None, device_ptr=None, stride=None, shape=None, fmt="mono8"):
    """lvk_image for a host array (H, W) uint8 — or for a device pointer with an explicit (H, W) shape and row stride.
    fmt: the pixel format the front-end was switched to (ImageProcessor.set_input_format); the host array is then what
    pixfmt_host_array describes and a device pointer's default stride is the format's row bytes.
    Returns (Image, keepalive): hold the second value until the call that consumes the image has returned."""
    if device_ptr is not None:
        h, w = shape
        return Image(int(device_ptr), int(w), int(h), int(stride if stride is not None else w * _PIX_ARRAY[fmt][2]), 1), None
    if fmt != "mono8":
        img = pixfmt_host_array(img, fmt)
        return Image(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], 0), img
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1:
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim != 2:
            raise ValueError("image must be a 2-D uint8 array")
    return Image(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], 0), img


class FeConfig(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("pyramid_levels", C.c_int), ("patch_size", C.c_int),
                ("max_iteration", C.c_int), ("track_precision", C.c_double), ("max_features_num", C.c_int),
                ("min_distance", C.c_int), ("flag_equalize", C.c_int), ("pub_frequency", C.c_int),
                ("distortion_model", C.c_int), ("intrinsics", C.c_double * 4), ("distortion", C.c_double * 4),
                ("R_cam_imu", C.c_double * 9)]


# lvk_match_query / lvk_match_result / lvk_landmark_match / lvk_match_options of include/lvk_c.h, and the LVK_MATCH_* status codes by name
MATCH_QUERY = np.dtype([("x", np.float32), ("y", np.float32), ("radius", np.float32), ("pad", np.float32)])
MATCH_RESULT = np.dtype([("cand", np.int32), ("dist", np.int32), ("second", np.int32), ("n_window", np.int32), ("status", np.int32), ("pad", np.int32)])
LANDMARK_MATCH = np.dtype([("status", np.int32), ("dist", np.int32), ("second", np.int32), ("n_window", np.int32), ("px", np.float32, 2), ("und", np.float32, 2)])
MATCH_OK, MATCH_NO_CANDIDATE, MATCH_TOO_FAR, MATCH_AMBIGUOUS, MATCH_CONFLICT = 0, 1, 2, 3, 4


class MatchOptions(C.Structure):
    _fields_ = [("max_candidates", C.c_int), ("quality", C.c_double), ("min_distance", C.c_double), ("max_dist", C.c_int), ("ratio_pct", C.c_int)]


# lvk_align_match / lvk_align_pair / lvk_align_model / lvk_align_hyp / lvk_align_result / lvk_align_options of include/lvk_c.h, the
# LVK_ALIGN_* status codes and the seed a 0 stands for
ALIGN_MATCH = np.dtype([("X", np.float64, 3), ("u", np.float64), ("v", np.float64)])
ALIGN_PAIR = np.dtype([("i", np.int32), ("j", np.int32)])
ALIGN_MODEL = np.dtype([("count", np.int32), ("root", np.int32), ("c", np.float64), ("s", np.float64), ("t", np.float64, 3)])
ALIGN_HYP = np.dtype([("n_models", np.int32), ("pad", np.int32), ("m", ALIGN_MODEL, 2)])
ALIGN_RESULT = np.dtype([("status", np.int32), ("n_inliers", np.int32), ("hyp", np.int32), ("root", np.int32), ("pair_i", np.int32), ("pair_j", np.int32),
                         ("iters", np.int32), ("pad", np.int32), ("c", np.float64), ("s", np.float64), ("t", np.float64, 3),
                         ("c0", np.float64), ("s0", np.float64), ("t0", np.float64, 3), ("A", np.float64, (4, 4)), ("rms", np.float64)])
ALIGN_OK, ALIGN_NO_MODEL, ALIGN_FEW_INLIERS, ALIGN_SINGULAR = 0, 1, 2, 3
ALIGN_DEFAULT_SEED = 0xFFFFFFFF
ALIGN_MAX_MATCHES, ALIGN_MAX_PAIRS = 1024, 4096


class AlignOptions(C.Structure):
    _fields_ = [("thresh", C.c_double), ("min_depth", C.c_double), ("min_dz", C.c_double), ("min_inliers", C.c_int), ("max_refine_iters", C.c_int)]


# lvk_map_sel / lvk_map_info / lvk_map_match / lvk_map_camera / lvk_map_select_options of include/lvk_c.h, the LVK_MAP_* status codes, the bit
# a selected point carries in its status byte and the two caps
MAP_SEL = np.dtype([("index", np.int32), ("cell", np.int32), ("x", np.float32), ("y", np.float32), ("radius", np.float32), ("depth", np.float32)])
MAP_INFO = np.dtype([("n_selected", np.int32), ("n_visible", np.int32), ("n_behind", np.int32), ("n_far", np.int32), ("n_outside", np.int32),
                     ("n_candidates", np.int32), ("pad", np.int32, 2)])
MAP_MATCH = np.dtype([("index", np.int32), ("cell", np.int32), ("q", MATCH_QUERY), ("depth", np.float32), ("pad", np.float32), ("m", LANDMARK_MATCH)])
MAP_VISIBLE, MAP_BEHIND, MAP_FAR, MAP_OUTSIDE = 0, 1, 2, 3
MAP_SELECTED = 0x80
MAP_MAX_POINTS, MAP_MAX_QUERIES = 1 << 20, 1024
# lvk_map_obs_info (lvk_map_gather_obs) and lvk_localise_info (lvk_vio_localise_map) of include/lvk_c.h, and the LVK_LOCALISE_* status codes
MAP_OBS_INFO = np.dtype([("n_ok", np.int32), ("n_bad", np.int32), ("pad", np.int32, 2)])
LOCALISE_INFO = np.dtype([("status", np.int32), ("n_ok", np.int32), ("n_bad", np.int32), ("pad", np.int32), ("clone_id", np.int64), ("map", MAP_INFO),
                          ("R_wc", np.float64, (3, 3)), ("p_wc", np.float64, 3), ("cov_cam", np.float64, (6, 6))])
LOCALISE_QUEUED, LOCALISE_NO_CLONE = 0, 1


# lvk_global_match / lvk_global_info / lvk_reloc_match of include/lvk_c.h and the caps of lvk_orb_match_global
GLOBAL_MATCH = np.dtype([("cand", np.int32), ("index", np.int32), ("dist", np.int32), ("second", np.int32)])
GLOBAL_INFO = np.dtype([("n_ok", np.int32), ("n_no_candidate", np.int32), ("n_too_far", np.int32), ("n_ambiguous", np.int32), ("n_conflict", np.int32),
                        ("n_selected", np.int32), ("pad", np.int32, 2)])
RELOC_MATCH = np.dtype([("cand", np.int32), ("index", np.int32), ("dist", np.int32), ("second", np.int32), ("px", np.float32, 2), ("und", np.float32, 2),
                        ("inlier", np.int32), ("pad", np.int32)])
GLOBAL_MAX_CAND, GLOBAL_MAX_MATCHES = 4096, 1024


# lvk_map_build_info / lvk_map_build_options of include/lvk_c.h and the LVK_MAPB_* status codes
MAP_BUILD_INFO = np.dtype([("n_kept", np.int32), ("n_bad", np.int32), ("n_uncertain", np.int32), ("n_out_of_range", np.int32), ("n_duplicate", np.int32),
                           ("pad", np.int32, 3)])
MAPB_KEPT, MAPB_BAD, MAPB_UNCERTAIN, MAPB_OUT_OF_RANGE, MAPB_DUPLICATE = 0, 1, 2, 3, 4


# lvk_align3d_match / lvk_align3d_hyp / lvk_align3d_options of include/lvk_c.h (lvk_align_ransac_3d; pairs, result and statuses are ALIGN_*)
ALIGN3D_MATCH = np.dtype([("X", np.float64, 3), ("Y", np.float64, 3)])
ALIGN3D_HYP = np.dtype([("n_models", np.int32), ("count", np.int32), ("pad", np.int32, 2), ("c", np.float64), ("s", np.float64), ("t", np.float64, 3)])


class Align3dOptions(C.Structure):
    _fields_ = [("thresh", C.c_double), ("min_rho", C.c_double), ("min_inliers", C.c_int), ("pad", C.c_int)]


class MapBuildOptions(C.Structure):
    _fields_ = [("max_score", C.c_double), ("r_dup", C.c_double), ("dup_max_dist", C.c_int), ("pad", C.c_int)]


class MapCamera(C.Structure):
    _fields_ = [("intr", C.c_double * 4), ("model", C.c_int), ("width", C.c_int), ("height", C.c_int), ("pad", C.c_int), ("dist", C.c_double * 4)]


class MapSelectOptions(C.Structure):
    _fields_ = [("min_depth", C.c_double), ("max_depth", C.c_double), ("max_r2", C.c_double), ("margin", C.c_double), ("k_sigma", C.c_double),
                ("sigma_px", C.c_double), ("r_min", C.c_double), ("r_max", C.c_double), ("rows", C.c_int), ("cols", C.c_int), ("quota", C.c_int), ("pad", C.c_int)]


def lib():
    """Load liblvk_hip.so.  Fails loudly when the HIP extension has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_SO):
            raise LvkError(f"{_SO} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(_SO)
        vp, i, d, sz = C.c_void_p, C.c_int, C.c_double, C.c_size_t
        pi = C.POINTER(C.c_int)
        sig = {
            "lvk_runtime_env": ([C.c_uint, i], C.c_uint),
            "lvk_context_create": ([i, C.POINTER(vp)], i), "lvk_context_destroy": ([vp], None),
            "lvk_context_set_stream": ([vp, vp], i), "lvk_sync": ([vp], i),
            "lvk_last_error": ([vp], C.c_char_p), "lvk_version": ([], C.c_char_p),
            "lvk_malloc": ([vp, sz, C.POINTER(vp)], i), "lvk_free": ([vp, vp], i),
            "lvk_memcpy_h2d": ([vp, vp, vp, sz], i), "lvk_memcpy_d2h": ([vp, vp, vp, sz], i), "lvk_memset": ([vp, vp, i, sz], i),
            "lvk_clahe_u8": ([vp, vp, i, i, i, vp, i, d, i, i], i),
            "lvk_pyramid_create": ([vp, i, i, i, i, C.POINTER(vp)], i), "lvk_pyramid_destroy": ([vp], None),
            "lvk_pyramid_build": ([vp, vp, vp, i], i), "lvk_pyramid_build_clahe": ([vp, vp, vp, i, d, i, i], i),
            "lvk_pyramid_levels": ([vp], i),
            "lvk_pyramid_level": ([vp, i, pi, pi, pi, pi, pi, C.POINTER(vp), C.POINTER(vp)], i),
            "lvk_orb_prepare": ([vp, vp, vp, vp], i), "lvk_min_eigen_map": ([vp, vp, vp], i),
            "lvk_good_features": ([vp, vp, vp, i, d, d, vp, i, vp], i),
            "lvk_good_features_from_map": ([vp, vp, vp, i, i, i, d, d, vp, i, vp], i),
            "lvk_lk_track": ([vp, vp, vp, vp, vp, vp, i, i, d, vp], i),
            "lvk_orb_describe": ([vp, vp, vp, i, i, vp, i, vp, vp], i),
            "lvk_hamming256_rows": ([vp, vp, vp, i, vp], i),
            "lvk_undistort_points": ([vp, vp, i, vp, i, vp, vp, vp], i),
            "lvk_find_fundamental_mask": ([vp, vp, vp, i, d, d, vp, vp], i),
            "lvk_find_fundamental": ([vp, vp, vp, i, d, d, vp, vp, vp], i),
            "lvk_ransac_fundamental": ([vp, vp, vp, i, d, d, i, vp, vp], i),
            "lvk_orb_match_guided": ([vp, vp, vp, i, vp, vp, i, i, i, vp], i),
            "lvk_align_ransac_2pt": ([vp, vp, i, vp, i, vp, vp, C.POINTER(AlignOptions), vp, vp, vp], i),
            "lvk_align_draw_pairs": ([i, i, C.c_uint32, vp], i),
            "lvk_map_select_queries": ([vp, vp, vp, vp, i, C.POINTER(MapCamera), vp, vp, vp, vp, C.POINTER(MapSelectOptions), vp, vp, vp, vp, vp], i),
            "lvk_map_build": ([vp, vp, vp, vp, vp, i, C.POINTER(MapBuildOptions), vp, vp, vp, vp, vp, vp], i),
            "lvk_orb_match_global": ([vp, vp, i, vp, i, i, i, i, vp, vp, vp], i),
            "lvk_align_ransac_3d": ([vp, vp, i, vp, i, C.POINTER(Align3dOptions), vp, vp, vp], i),
            "lvk_align_invert": ([vp, vp], i),
            "lvk_map_transform": ([vp, vp, vp, vp, i, vp, vp, vp, vp, vp], i),
            "lvk_predict_homography": ([vp, i, d, d, vp, vp, vp], i),
            "lvk_frontend_create": ([vp, C.POINTER(FeConfig), C.POINTER(vp)], i), "lvk_frontend_destroy": ([vp], None),
            "lvk_frontend_process": ([vp, C.POINTER(Image), d, vp, i, vp, i, pi, pi], i),
            "lvk_frontend_tracks": ([vp, vp, vp, vp, vp, vp, i, pi], i),
            "lvk_frontend_new_pts": ([vp, vp, i, pi], i), "lvk_frontend_state": ([vp], i),
            "lvk_frontend_set_mask": ([vp, C.POINTER(Image)], i), "lvk_frontend_has_mask": ([vp], i),
            "lvk_image_to_gray": ([vp, vp, i, i, i, i, i, vp, i], i),
            "lvk_frontend_set_input_format": ([vp, i, i], i), "lvk_frontend_input_format": ([vp], i),
            "lvk_frontend_match_landmarks": ([vp, vp, vp, i, C.POINTER(MatchOptions), vp, pi], i),
            "lvk_frontend_align_landmarks": ([vp, vp, i, vp, vp, C.POINTER(AlignOptions), i, C.c_uint32, vp, vp], i),
            "lvk_frontend_set_map": ([vp, vp, vp, vp, i], i), "lvk_frontend_map_size": ([vp], i),
            "lvk_frontend_build_map": ([vp, vp, vp, vp, vp, i, C.POINTER(MapBuildOptions), vp, i, vp], i),
            "lvk_frontend_match_map": ([vp, vp, vp, vp, vp, C.POINTER(MapSelectOptions), C.POINTER(MatchOptions), vp, i, pi, vp], i),
            "lvk_frontend_relocalise_map": ([vp, vp, vp, C.POINTER(MatchOptions), C.POINTER(AlignOptions), i, i, C.c_uint32, vp, vp, i, pi, vp], i),
            "lvk_frontend_merge_map": ([vp, vp, vp, vp, i, vp, vp, C.POINTER(MatchOptions), C.POINTER(Align3dOptions), i, C.c_uint32, C.POINTER(MapBuildOptions), vp, vp, i, vp, vp], i),
            "lvk_frontend_lk_stats": ([vp, vp, vp], i),
            "lvk_frontend_msg_stats": ([vp, vp, vp], i),
            "lvk_frontend_profile_enable": ([vp, C.c_uint], i), "lvk_frontend_profile_read": ([vp, vp, vp, i], i),
            "lvk_frontend_stage_name": ([i], C.c_char_p),
            "lvk_ekf_camera_pose_cov": ([vp, vp, i, i, vp, vp, vp, vp], i),
            "lvk_map_gather_obs": ([vp, vp, i, vp, vp, i, vp, d, vp, vp, vp], i),
            "lvk_vio_localise_map": ([vp, vp, vp, C.c_int64, d, d, C.POINTER(MapSelectOptions), C.POINTER(MatchOptions), C.c_int64, vp], i),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _LIB = L
    return _LIB


def _p(a):
    if a is None:
        return None
    if isinstance(a, DeviceBuffer):
        return C.c_void_p(a.ptr)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):          # torch tensor on the GPU
        return C.c_void_p(a.data_ptr())
    raise TypeError(type(a))


class Context:
    """lvk_context: one GPU, one stream."""

    def __init__(self, device=0, stream=None):
        L = lib()
        h = C.c_void_p()
        st = L.lvk_context_create(device, C.byref(h))
        if st != 0:
            raise LvkError(f"lvk_context_create failed with status {st}: no usable gfx950 device (there is no CPU fallback)")
        self.h = h
        self._bufs = []
        self._children = weakref.WeakSet()      # front-ends / filters created on this context: closed before it
        if stream is not None:
            self.check(L.lvk_context_set_stream(self.h, C.c_void_p(stream)))

    def check(self, st):
        if st != 0:
            raise LvkError(f"lvk status {st}: {lib().lvk_last_error(self.h).decode()}")

    def sync(self):
        self.check(lib().lvk_sync(self.h))

    @property
    def stream(self):
        """the hipStream_t (as an integer) the context's calls are ordered on"""
        L = lib()
        L.lvk_context_get_stream.argtypes = [C.c_void_p]; L.lvk_context_get_stream.restype = C.c_void_p
        return L.lvk_context_get_stream(self.h) or 0

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        b = DeviceBuffer(self, arr.nbytes)
        if arr.nbytes:
            self.check(lib().lvk_memcpy_h2d(self.h, C.c_void_p(b.ptr), _p(arr), arr.nbytes))
        return b

    def to_host(self, buf, dtype, shape):
        out = np.empty(shape, dtype)
        if out.nbytes:
            self.check(lib().lvk_memcpy_d2h(self.h, _p(out), C.c_void_p(buf.ptr if isinstance(buf, DeviceBuffer) else buf), out.nbytes))
        return out

    def adopt(self, obj):
        self._children.add(obj)

    def close(self):
        if self.h:
            for o in sorted(list(self._children), key=lambda o: getattr(o, "_close_order", 1)):
                try:
                    o.close()
                except Exception:
                    pass
            lib().lvk_sync(self.h)
            lib().lvk_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        p = C.c_void_p()
        ctx.check(lib().lvk_malloc(ctx.h, max(int(nbytes), 1), C.byref(p)))
        self.ptr = p.value
        self.nbytes = nbytes

    def free(self):
        if self.ptr and self.ctx.h:
            lib().lvk_free(self.ctx.h, C.c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
