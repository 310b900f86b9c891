"""LarVio — host-side mirror of larvio::LarVio over the C ABI (include/lvk_c.h, back-end section).

Same surface as the reference class (include/larvio/larvio.h:37-90): construct with the configuration,
``initialize()``, then ``processFeatures(msg, imu_buffer)`` per feature message; getters for pose / velocity /
covariance / sliding window / map points.  The arithmetic runs in liblvk_hip.so on the GPU; like the reference,
``processFeatures`` erases the IMU samples it consumed from the caller's buffer (larvio.cpp:511-512).
"""
import ctypes as C
import os
import numpy as np
from ._lib import lib, _p, Context, LvkError, IMU, OBS

CLONE = np.dtype([("id", np.int64), ("time", np.float64), ("dt", np.float64), ("q", np.float64, 4), ("p", np.float64, 3),
                  ("p_fej", np.float64, 3), ("R_b2c", np.float64, 9), ("t_c_b", np.float64, 3), ("q_cam", np.float64, 4),
                  ("p_cam", np.float64, 3)])

# lvk_keyframe (include/lvk_c.h): one pruned clone
KEYFRAME = np.dtype([("id", np.int64), ("to_id", np.int64), ("time", np.float64), ("to_time", np.float64), ("q", np.float64, 4), ("p", np.float64, 3),
                     ("rel_q", np.float64, 4), ("rel_p", np.float64, 3), ("cov_abs", np.float64, (6, 6)), ("cov_rel", np.float64, (6, 6))])

# lvk_fix / lvk_fix_report (include/lvk_c.h)
FIX = np.dtype([("tag", np.int64), ("kind", np.int32), ("pad", np.int32), ("clone_id", np.int64), ("time", np.float64), ("p", np.float64, 3), ("q", np.float64, 4),
                ("lever", np.float64, 3), ("cov", np.float64, (6, 6))])
FIX_REPORT = np.dtype([("tag", np.int64), ("kind", np.int32), ("status", np.int32), ("gamma", np.float64), ("clone_i", np.int64), ("clone_j", np.int64),
                       ("a", np.float64)])
FIX_POSITION, FIX_POSE = 0, 1
FIX_APPLIED, FIX_GATED, FIX_NOT_PD, FIX_STALE, FIX_NO_CLONE = 0, 1, 2, 3, 4
# lvk_landmark_report (include/lvk_c.h; the observation record lvk_landmark_obs is ops.LANDMARK_OBS)
LANDMARK_REPORT = np.dtype([("tag", np.int64), ("status", np.int32), ("n_obs", np.int32), ("clone_id", np.int64), ("n_used", np.int32), ("n_gated", np.int32),
                            ("n_behind", np.int32), ("pad0", np.int32), ("gamma", np.float64)])
LANDMARKS_APPLIED, LANDMARKS_ALL_REJECTED, LANDMARKS_NOT_PD, LANDMARKS_STALE, LANDMARKS_NO_CLONE = 0, 1, 2, 3, 4

_CFG_INT = ["if_fej", "estimate_extrin", "estimate_td", "if_zupt_valid", "sw_size", "max_track_len", "least_observation_number",
            "max_features_in_one_grid", "aug_grid_rows", "aug_grid_cols", "width", "height"]
_CFG_DBL = ["td", "pub_frequency", "imu_rate", "noise_gyro", "noise_acc", "noise_gyro_bias", "noise_acc_bias", "noise_feature",
            "initial_covariance_orientation", "initial_covariance_velocity", "initial_covariance_position",
            "initial_covariance_gyro_bias", "initial_covariance_acc_bias", "initial_covariance_extrin_rot",
            "initial_covariance_extrin_trans", "rotation_threshold", "translation_threshold", "tracking_rate_threshold",
            "feature_translation_threshold", "zupt_max_feature_dis", "zupt_noise_v", "zupt_noise_p", "zupt_noise_q", "static_duration"]


class EkfConfig(C.Structure):
    _fields_ = ([(k, C.c_int) for k in _CFG_INT] + [("intrinsics", C.c_double * 4), ("T_cam_imu", C.c_double * 16)] +
                [(k, C.c_double) for k in _CFG_DBL] +
                [("feature_idp_dim", C.c_int), ("use_schmidt", C.c_int), ("calib_imu_instrinsic", C.c_int), ("max_features", C.c_int),
                 ("legacy_grid", C.c_int), ("reserved0", C.c_int)])


_sig_done = False


class InitReport(C.Structure):
    """lvk_init_report (include/lvk_c.h)"""
    _fields_ = [("valid", C.c_int), ("message", C.c_int), ("attempts", C.c_int), ("ransac_calls", C.c_int), ("l", C.c_int), ("n_points", C.c_int), ("erase", C.c_int), ("pad", C.c_int),
                ("state_time", C.c_double), ("scale", C.c_double), ("rel_R", C.c_double * 9), ("rel_T", C.c_double * 3), ("sfm_R", C.c_double * 99), ("sfm_T", C.c_double * 33),
                ("bg", C.c_double * 3), ("g", C.c_double * 3), ("q", C.c_double * 4), ("v", C.c_double * 3)]


def _L():
    global _sig_done
    L = lib()
    if not _sig_done:
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        pi = C.POINTER(C.c_int)
        L.lvk_ekf_compress_qr.argtypes = [vp, vp, i, i, i, vp, pi]; L.lvk_ekf_compress_qr.restype = i
        L.lvk_ekf_update.argtypes = [vp, vp, i, i, vp, i, i, vp, d, vp]; L.lvk_ekf_update.restype = i
        L.lvk_ekf_compress_qr_groups.argtypes = [vp, vp, i, i, i, vp, i, vp, vp, vp, pi]; L.lvk_ekf_compress_qr_groups.restype = i
        L.lvk_ekf_qr_plan.argtypes = [i, i, vp, vp, vp, vp, i, vp, i, vp, vp, i, pi]; L.lvk_ekf_qr_plan.restype = i
        L.lvk_dgemm.argtypes = [vp, i, i, i, i, i, d, vp, i, vp, i, d, vp, i]; L.lvk_dgemm.restype = i
        L.lvk_dgemm_ex.argtypes = [vp, i, i, i, i, i, d, vp, i, vp, i, d, vp, i, d, vp, i, vp, i, vp]; L.lvk_dgemm_ex.restype = i
        L.lvk_chol_solve.argtypes = [vp, vp, i, i, vp, i, i, vp]; L.lvk_chol_solve.restype = i
        L.lvk_ekf_cov_propagate_augment.argtypes = [vp, vp, i, vp, i, i, i, i, vp, vp]; L.lvk_ekf_cov_propagate_augment.restype = i
        L.lvk_ekf_cov_gather.argtypes = [vp, vp, i, vp, i, vp, i]; L.lvk_ekf_cov_gather.restype = i
        L.lvk_ekf_cov_reanchor.argtypes = [vp, vp, i, i, vp, i]; L.lvk_ekf_cov_reanchor.restype = i
        L.lvk_ekf_cov_append_features.argtypes = [vp, vp, i, i, i, vp, i, vp, vp, vp, d, vp]; L.lvk_ekf_cov_append_features.restype = i
        L.lvk_ekf_create.argtypes = [vp, C.POINTER(EkfConfig), C.POINTER(vp)]; L.lvk_ekf_create.restype = i
        L.lvk_ekf_destroy.argtypes = [vp]; L.lvk_ekf_destroy.restype = None
        L.lvk_ekf_process.argtypes = [vp, d, vp, i, vp, i, pi, pi]; L.lvk_ekf_process.restype = i
        L.lvk_ekf_set_state.argtypes = [vp, d, vp, vp, vp, vp, vp, vp, vp]; L.lvk_ekf_set_state.restype = i
        L.lvk_ekf_dim.argtypes = [vp]; L.lvk_ekf_dim.restype = i
        L.lvk_ekf_is_initialized.argtypes = [vp]; L.lvk_ekf_is_initialized.restype = i
        L.lvk_ekf_take_off_stamp.argtypes = [vp]; L.lvk_ekf_take_off_stamp.restype = C.c_double
        L.lvk_ekf_take_lost_features.argtypes = [vp, vp, vp, i]; L.lvk_ekf_take_lost_features.restype = i
        L.lvk_ekf_get_feature_cov.argtypes = [vp, vp, vp, vp, vp, i, pi]; L.lvk_ekf_get_feature_cov.restype = i
        L.lvk_ekf_get_feature_rel.argtypes = [vp, C.c_int64, vp, vp, vp, vp, i, pi]; L.lvk_ekf_get_feature_rel.restype = i
        L.lvk_ekf_set_lost_feature_cov.argtypes = [vp, i]; L.lvk_ekf_set_lost_feature_cov.restype = i
        L.lvk_ekf_take_lost_features_cov.argtypes = [vp, vp, vp, vp, i]; L.lvk_ekf_take_lost_features_cov.restype = i
        L.lvk_ekf_set_msckf_points.argtypes = [vp, i]; L.lvk_ekf_set_msckf_points.restype = i
        L.lvk_ekf_take_msckf_points.argtypes = [vp, vp, vp, vp, vp, i]; L.lvk_ekf_take_msckf_points.restype = i
        L.lvk_ekf_set_keyframe_export.argtypes = [vp, i]; L.lvk_ekf_set_keyframe_export.restype = i
        L.lvk_ekf_take_keyframes.argtypes = [vp, vp, i]; L.lvk_ekf_take_keyframes.restype = i
        L.lvk_ekf_get_window_cov.argtypes = [vp, vp, vp, vp, i, pi]; L.lvk_ekf_get_window_cov.restype = i
        L.lvk_ekf_add_fix.argtypes = [vp, vp]; L.lvk_ekf_add_fix.restype = i
        L.lvk_ekf_set_fix_options.argtypes = [vp, d, d]; L.lvk_ekf_set_fix_options.restype = i
        L.lvk_ekf_take_fix_reports.argtypes = [vp, vp, i]; L.lvk_ekf_take_fix_reports.restype = i
        L.lvk_ekf_fix_stats.argtypes = [vp, vp]; L.lvk_ekf_fix_stats.restype = None
        L.lvk_ekf_add_landmark_obs.argtypes = [vp, C.c_int64, C.c_int64, d, vp, i]; L.lvk_ekf_add_landmark_obs.restype = i
        L.lvk_ekf_set_landmark_options.argtypes = [vp, d, d]; L.lvk_ekf_set_landmark_options.restype = i
        L.lvk_ekf_take_landmark_reports.argtypes = [vp, vp, i]; L.lvk_ekf_take_landmark_reports.restype = i
        L.lvk_ekf_landmark_stats.argtypes = [vp, vp]; L.lvk_ekf_landmark_stats.restype = None
        L.lvk_ekf_get_state.argtypes = [vp, vp]; L.lvk_ekf_get_state.restype = i
        L.lvk_ekf_get_cov.argtypes = [vp, vp]; L.lvk_ekf_get_cov.restype = i
        L.lvk_ekf_get_cov_imu.argtypes = [vp, i, vp]; L.lvk_ekf_get_cov_imu.restype = i
        L.lvk_ekf_set_cov.argtypes = [vp, vp, i]; L.lvk_ekf_set_cov.restype = i
        L.lvk_ekf_set_indefinite_policy.argtypes = [vp, i]; L.lvk_ekf_set_indefinite_policy.restype = i
        L.lvk_ekf_indefinite_fallbacks.argtypes = [vp]; L.lvk_ekf_indefinite_fallbacks.restype = C.c_long
        L.lvk_ekf_last_update.argtypes = [vp, pi, pi, vp, vp, vp, vp]; L.lvk_ekf_last_update.restype = i
        L.lvk_ekf_update_ldlt.argtypes = [vp, vp, i, i, vp, i, i, vp, d, vp, vp]; L.lvk_ekf_update_ldlt.restype = i
        L.lvk_ekf_update_ldlt_perm.argtypes = [vp, vp, i, i, vp, i, i, vp, d, vp, vp, vp]; L.lvk_ekf_update_ldlt_perm.restype = i
        L.lvk_ekf_get_imu_intrinsics.argtypes = [vp, vp]; L.lvk_ekf_get_imu_intrinsics.restype = i
        L.lvk_ekf_set_imu_intrinsics.argtypes = [vp, vp]; L.lvk_ekf_set_imu_intrinsics.restype = i
        L.lvk_ekf_get_clones.argtypes = [vp, vp, i]; L.lvk_ekf_get_clones.restype = i
        L.lvk_ekf_get_features.argtypes = [vp, vp, vp, vp, i]; L.lvk_ekf_get_features.restype = i
        L.lvk_ekf_counters.argtypes = [vp, vp]; L.lvk_ekf_counters.restype = None
        L.lvk_ekf_init_report.argtypes = [vp, vp]; L.lvk_ekf_init_report.restype = C.c_int
        L.lvk_ekf_profile.argtypes = [vp, i, vp]; L.lvk_ekf_profile.restype = i
        L.lvk_ekf_set_shard.argtypes = [vp, i, i, vp, vp]; L.lvk_ekf_set_shard.restype = i
        L.lvk_ekf_shard_stats.argtypes = [vp, vp]; L.lvk_ekf_shard_stats.restype = None
        L.lvk_triangulate.argtypes = [vp, vp, vp, i, i, vp, pi, vp, vp, vp, vp]; L.lvk_triangulate.restype = i
        L.lvk_ekf_gate_and_stack.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, i, i, i, d, vp, vp, i, pi, vp, vp]; L.lvk_ekf_gate_and_stack.restype = i
        L.lvk_ekf_feature_rows.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, i, vp, i, i, i, i, i, d, i, vp, vp, vp, vp, i, i, vp, pi]; L.lvk_ekf_feature_rows.restype = i
        L.lvk_shard_pack_stage.argtypes = [vp, i, vp, i, vp, i, i, vp, i, C.c_size_t, i, vp, C.c_size_t]; L.lvk_shard_pack_stage.restype = i
        L.lvk_shard_unpack_stage.argtypes = [vp, vp, C.c_size_t, vp, i, i, i, C.c_size_t, vp, i, i, vp, vp, vp, i, vp]; L.lvk_shard_unpack_stage.restype = i
        _sig_done = True
    return L


# ---------------------------------------------------------------- stage-level wrappers (numpy in / numpy out)
POSE = np.dtype([("R", np.float64, 9), ("t", np.float64, 3)])
MSCKF_FEATURE = np.dtype([("p_w", np.float64, 3), ("n_obs", np.int32), ("obs_off", np.int32)])


def triangulate(ctx, poses, obs, use_position=False, position_in=None):
    """Feature::initializePosition for one feature (feature.hpp:383-552).  Returns (ok, position, solution, inv_depth, obs_anchor)."""
    poses = np.ascontiguousarray(poses, POSE); obs = np.ascontiguousarray(obs, np.float64)
    pin = np.ascontiguousarray(position_in if position_in is not None else np.zeros(3), np.float64)
    ok = C.c_int(0); pos = np.zeros(3); sol = np.zeros(3); idp = np.zeros(1); oa = np.zeros(3)
    ctx.check(_L().lvk_triangulate(ctx.h, _p(poses), _p(obs), len(poses), int(use_position), _p(pin), C.byref(ok), _p(pos), _p(sol), _p(idp), _p(oa)))
    return bool(ok.value), pos, sol, float(idp[0]), oa


def gate_and_stack(ctx, clones, feats, clone_rank, obs, obs_vel, P, sigma2, if_fej=1, estimate_td=1):
    """featureJacobian_msckf + gatingTest + stacking for a batch of MSCKF features.  feats: list of (p_w, n_obs, obs_off).
    Returns (H (rows x N), r, gamma[n_feats], accept[n_feats])."""
    clones = np.ascontiguousarray(clones, CLONE)
    fa = np.zeros(len(feats), MSCKF_FEATURE)
    for k, (pw, n, off) in enumerate(feats):
        fa[k]["p_w"] = pw; fa[k]["n_obs"] = n; fa[k]["obs_off"] = off
    cr = np.ascontiguousarray(clone_rank, np.int32); obs = np.ascontiguousarray(obs, np.float64); ov = np.ascontiguousarray(obs_vel, np.float64)
    P = np.ascontiguousarray(P, np.float64); N = P.shape[0]
    cap = int(sum(2 * n - 3 for _, n, _ in feats)) + 1
    H = np.zeros((cap, N)); r = np.zeros(cap); rows = C.c_int(0); gamma = np.zeros(len(feats)); acc = np.zeros(len(feats), np.int32)
    ctx.check(_L().lvk_ekf_gate_and_stack(ctx.h, _p(clones), len(clones), _p(fa), len(fa), _p(cr), _p(obs), _p(ov), _p(P), N, int(if_fej), int(estimate_td),
                                          float(sigma2), _p(H), _p(r), cap, C.byref(rows), _p(gamma), _p(acc)))
    return H[:rows.value].copy(), r[:rows.value].copy(), gamma, acc.astype(bool)


FEATURE_JOB = np.dtype([("type", np.int32), ("n_obs", np.int32), ("obs_off", np.int32), ("anchor_rank", np.int32), ("fcol", np.int32), ("gate", np.int32),
                        ("tri_pending", np.int32), ("pad", np.int32), ("p_w", np.float64, 3), ("p_fej", np.float64, 3), ("inv_depth", np.float64),
                        ("obs_anchor", np.float64, 3)])
FEATURE_RESULT = np.dtype([("gamma", np.float64), ("h2", np.float64), ("rows", np.int32), ("first_row", np.int32), ("c", np.int32), ("accept", np.int32)])
FJ_MSCKF, FJ_EKF_NEW, FJ_EKF_TRACKED = 0, 1, 2
FR_GENERAL, FR_STRIDE, FR_DIRECT, FR_DEVICE_ZERO = 1, 2, 4, 8


def feature_job_cols(job):
    """compact columns of a job: 7 (extrinsics + td) + 6 per observing clone (+ the anchor's 6 and the feature column for EKF jobs)"""
    M = int(job["n_obs"])
    return 7 + 6 * M if job["type"] == FJ_MSCKF else 7 + 6 + 6 * M + 1


def feature_rows(ctx, clones, jobs, clone_rank, obs, obs_vel, P, ldp=None, leg_dim=22, if_fej=1, estimate_td=1, sigma2=0.008 ** 2, mode=0,
                 cams=None, H=None, r=None):
    """lvk_ekf_feature_rows: the filter's per-feature row stage for a batch of FEATURE_JOB records.  P: N x N, or a whole row-major
    buffer of ldp columns (its first N x N block is P).  H (rows x ldh) and r: the dense output buffers, read first and returned with
    the written rows (default: one row per candidate row, ldh = N, NaN-filled).  Returns (results, blocks, ccols, H, r, rows_out):
    blocks[j] = job j's compact [G | r] (2M x (c + 1)), ccols[j] = its column map."""
    clones = np.ascontiguousarray(clones, CLONE); jobs = np.ascontiguousarray(jobs, FEATURE_JOB)
    cr = np.ascontiguousarray(clone_rank, np.int32); obs = np.ascontiguousarray(obs, np.float64); ov = np.ascontiguousarray(obs_vel, np.float64)
    P = np.ascontiguousarray(P, np.float64)
    N = P.shape[0]
    if ldp is None:
        ldp = P.shape[1]
    pose = np.ascontiguousarray(cams, POSE) if cams is not None else None
    if H is None:
        H = np.full((sum(2 * int(j["n_obs"]) - (3 if j["type"] == FJ_MSCKF else 0) for j in jobs if j["type"] != FJ_EKF_NEW), N), np.nan)
    H = np.ascontiguousarray(H, np.float64)
    r = np.full(H.shape[0], np.nan) if r is None else np.ascontiguousarray(r, np.float64)
    res = np.zeros(len(jobs), FEATURE_RESULT)
    cols = [feature_job_cols(j) for j in jobs]
    blocks = np.zeros(sum(2 * int(j["n_obs"]) * (c + 1) for j, c in zip(jobs, cols)))
    cc = np.zeros(sum(cols), np.int32); rows = C.c_int(0)
    ctx.check(_L().lvk_ekf_feature_rows(ctx.h, _p(clones), len(clones), _p(jobs), len(jobs), _p(cr), _p(obs), _p(ov), _p(pose) if pose is not None else None, len(cr),
                                        _p(P), N, int(ldp), int(leg_dim), int(if_fej), int(estimate_td), float(sigma2), int(mode), _p(res), _p(blocks), _p(cc),
                                        _p(H), H.shape[1], H.shape[0], _p(r), C.byref(rows)))
    bl, cl = [], []
    bo = co = 0
    for j, c in zip(jobs, cols):
        n = 2 * int(j["n_obs"]) * (c + 1)
        bl.append(blocks[bo:bo + n].reshape(2 * int(j["n_obs"]), c + 1)); cl.append(cc[co:co + c]); bo += n; co += c
    return res, bl, cl, H, r, rows.value


# The exchange step of the sharded update (wire layout: include/lvk_c.h, next to lvk_shard_pack_stage).
SHARD_HDR, SHARD_MAGIC = 256, 0x4c564b58
SHARD_META = np.dtype([("job_lo", np.int32), ("job_n", np.int32), ("k", np.int32), ("row_off", np.int32)])


def shard_pack(ctx, rank, X, rX, res, res_bytes, bytes_per_rank, fill=0, k=None, ncols=None):
    """lvk_shard_pack_stage: k_shard_pack on k rows of the row-major buffer X (its row length is ld; k defaults to its rows, ncols to
    ld), their residuals rX and the FEATURE_RESULT records res -> the rank's block (uint8, bytes_per_rank); bytes the kernel did not
    write hold `fill`."""
    X = np.ascontiguousarray(X, np.float64); rX = np.ascontiguousarray(rX, np.float64); res = np.ascontiguousarray(res, FEATURE_RESULT)
    if X.ndim != 2:
        raise ValueError("X must be a 2-D buffer (rows x ld)")
    k = X.shape[0] if k is None else int(k); ncols = X.shape[1] if ncols is None else int(ncols)
    if k > X.shape[0] or k > len(rX):
        raise ValueError("k exceeds the rows given")
    out = np.empty(max(int(bytes_per_rank), 0), np.uint8)
    ctx.check(_L().lvk_shard_pack_stage(ctx.h, int(rank), _p(X), X.shape[1], _p(rX), k, ncols, _p(res), len(res), int(res_bytes), int(fill), _p(out), int(bytes_per_rank)))
    return out


def shard_unpack(ctx, recv, metas, ncols, k_max, res_bytes, H, r, fout, fout_host=None, peer_fail=0, bytes_per_rank=None):
    """lvk_shard_unpack_stage: k_shard_unpack on the received image recv (world blocks) and the plan metas (SHARD_META).  H (rows x
    ld), r, fout and fout_host (FEATURE_RESULT arrays of one length; fout_host None = the kernel gets no mirror array) go to the device
    as given; peer_fail: the word's value before the launch, None = the kernel gets no word.
    -> (H, r, fout, fout_host or None, peer_fail or None) after the kernel."""
    recv = np.ascontiguousarray(recv, np.uint8); metas = np.ascontiguousarray(metas, SHARD_META)
    H = np.array(H, np.float64, order="C"); r = np.array(r, np.float64); fout = np.array(fout, FEATURE_RESULT)
    fh = None if fout_host is None else np.array(fout_host, FEATURE_RESULT)
    if H.ndim != 2 or len(r) != H.shape[0] or (fh is not None and len(fh) != len(fout)):
        raise ValueError("H must be rows x ld, r one entry per row, fout_host as long as fout")
    world = len(metas)
    bpr = recv.size // max(world, 1) if bytes_per_rank is None else int(bytes_per_rank)
    if bpr < 0 or recv.size < world * bpr:
        raise ValueError("recv is shorter than world * bytes_per_rank")
    word = None if peer_fail is None else np.array([peer_fail], np.int32)
    ctx.check(_L().lvk_shard_unpack_stage(ctx.h, _p(recv), bpr, _p(metas), world, int(ncols), int(k_max), int(res_bytes), _p(H), H.shape[1], H.shape[0], _p(r),
                                          _p(fout), _p(fh), len(fout), _p(word)))
    return H, r, fout, fh, (None if word is None else int(word[0]))


def _padded(X, ld, rows=None):
    """X (r x c) in a buffer of `rows` (>= r) rows of ld (>= c) doubles; everything outside X is NaN, as a padded buffer of the
    filter may hold anything there"""
    X = np.asarray(X, np.float64)
    buf = np.full((X.shape[0] if rows is None else rows, ld), np.nan)
    buf[:X.shape[0], :X.shape[1]] = X
    return buf


def dgemm(ctx, A, B, transa=False, transb=False, alpha=1.0, beta=0.0, Cin=None, ld=None):
    """C = alpha op(A) op(B) + beta Cin.  ld: A, B and C all stored with that leading dimension (NaN padding, as the filter's
    buffers); the whole C buffer (M x ld) is then returned, padding included."""
    A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64)
    M = A.shape[1] if transa else A.shape[0]; K = A.shape[0] if transa else A.shape[1]; N = B.shape[0] if transb else B.shape[1]
    Cm = np.zeros((M, N)) if Cin is None else np.array(Cin, np.float64, order="C")
    if ld is not None:
        A, B, Cm = _padded(A, ld), _padded(B, ld), _padded(Cm, ld)
    dA, dB, dC = ctx.to_device(A), ctx.to_device(B), ctx.to_device(Cm)
    ctx.check(_L().lvk_dgemm(ctx.h, int(transa), int(transb), M, N, K, alpha, _p(dA), A.shape[1], _p(dB), B.shape[1], beta, _p(dC), Cm.shape[1]))
    return ctx.to_host(dC, np.float64, Cm.shape)


def dgemm_ex(ctx, A, B, Cbuf, M, N, K, transa=False, transb=False, alpha=1.0, beta=0.0, diag_add=0.0, xin=None, xin_col=0, xout=None, xout_col=0,
             gate=None):
    """lvk_dgemm_ex on whole row-major buffers (leading dimension = row length; contents go to the device as they are).  xin: M doubles;
    xout: the M doubles the diverted column's buffer holds before the call; gate: two ints.  -> (C buffer, xout buffer or None)"""
    A = np.ascontiguousarray(A, np.float64); B = np.ascontiguousarray(B, np.float64); Cbuf = np.ascontiguousarray(Cbuf, np.float64)
    dA, dB, dC = ctx.to_device(A), ctx.to_device(B), ctx.to_device(Cbuf)
    dxi = ctx.to_device(np.ascontiguousarray(xin, np.float64)) if xin is not None else None
    dxo = ctx.to_device(np.ascontiguousarray(xout, np.float64)) if xout is not None else None
    dg = ctx.to_device(np.ascontiguousarray(gate, np.int32)) if gate is not None else None
    ctx.check(_L().lvk_dgemm_ex(ctx.h, int(transa), int(transb), M, N, K, alpha, _p(dA), A.shape[1], _p(dB), B.shape[1], beta, _p(dC), Cbuf.shape[1],
                                diag_add, _p(dxi), int(xin_col), _p(dxo), int(xout_col), _p(dg)))
    return ctx.to_host(dC, np.float64, Cbuf.shape), (ctx.to_host(dxo, np.float64, (len(xout),)) if xout is not None else None)


def chol_solve(ctx, Sbuf, m, Bbuf, nbcols):
    """lvk_chol_solve on whole row-major buffers (Sbuf: >= m rows, its row length is lds; Bbuf likewise with ldb).
    -> (S buffer, B buffer, (info[0], info[1])) after the call"""
    Sbuf = np.ascontiguousarray(Sbuf, np.float64); Bbuf = np.ascontiguousarray(Bbuf, np.float64)
    dS, dB = ctx.to_device(Sbuf), ctx.to_device(Bbuf)
    info = np.full(2, -1, np.int32)
    ctx.check(_L().lvk_chol_solve(ctx.h, _p(dS), Sbuf.shape[1], int(m), _p(dB), Bbuf.shape[1], int(nbcols), _p(info)))
    return ctx.to_host(dS, np.float64, Sbuf.shape), ctx.to_host(dB, np.float64, Bbuf.shape), (int(info[0]), int(info[1]))


INDEFINITE_FAIL, INDEFINITE_LDLT = 0, 1


def ekf_update(ctx, P, H, r, sigma2, ld=None):
    """ld: P and H stored with that leading dimension (NaN padding, as the filter's buffers); the whole P buffer (n x ld) is then
    returned, padding included."""
    P = np.array(P, np.float64, order="C"); H = np.ascontiguousarray(H, np.float64); r = np.ascontiguousarray(r, np.float64)
    n, m = P.shape[0], H.shape[0]
    if ld is not None:
        P, H = _padded(P, ld), _padded(H, ld)
    dP, dH, dr, ddx = ctx.to_device(P), ctx.to_device(H), ctx.to_device(r), ctx.alloc(8 * n)
    ctx.check(_L().lvk_ekf_update(ctx.h, _p(dP), P.shape[1], n, _p(dH), H.shape[1], m, _p(dr), sigma2, _p(ddx)))
    return ctx.to_host(ddx, np.float64, (n,)), ctx.to_host(dP, np.float64, P.shape)


def ekf_update_ldlt(ctx, P, H, r, sigma2, ld=None, with_perm=False):
    """lvk_ekf_update_ldlt: the same update through the pivoted LDL^T (S need not be positive definite).  Arguments as ekf_update;
    -> dx, P, (negative D entries, zero D entries) and, with_perm, the pivot order (row i of the factor = row perm[i] of S)."""
    P = np.array(P, np.float64, order="C"); H = np.ascontiguousarray(H, np.float64); r = np.ascontiguousarray(r, np.float64)
    n, m = P.shape[0], H.shape[0]
    if ld is not None:
        P, H = _padded(P, ld), _padded(H, ld)
    dP, dH, dr, ddx = ctx.to_device(P), ctx.to_device(H), ctx.to_device(r), ctx.alloc(8 * n)
    info = np.zeros(2, np.int32); perm = np.zeros(max(m, 1), np.int32)
    if with_perm:
        ctx.check(_L().lvk_ekf_update_ldlt_perm(ctx.h, _p(dP), P.shape[1], n, _p(dH), H.shape[1], m, _p(dr), sigma2, _p(ddx), _p(info), _p(perm)))
    else:
        ctx.check(_L().lvk_ekf_update_ldlt(ctx.h, _p(dP), P.shape[1], n, _p(dH), H.shape[1], m, _p(dr), sigma2, _p(ddx), _p(info)))
    out = (ctx.to_host(ddx, np.float64, (n,)), ctx.to_host(dP, np.float64, P.shape), (int(info[0]), int(info[1])))
    return out + (perm[:m].copy(),) if with_perm else out


# The structural covariance operations (lvk_ekf_cov_*).  Matrices are passed as whole row-major buffers: the leading dimension is
# the buffer's row length, and the output buffer's previous contents (padding, rows the operation must not touch) go to the device
# as they are.  Each returns the whole output buffer after the call.
def cov_propagate_augment(ctx, Pin, Pout, n_out, pose_rows, phi, q):
    Pin = np.ascontiguousarray(Pin, np.float64); Pout = np.ascontiguousarray(Pout, np.float64)
    phi = np.ascontiguousarray(phi, np.float64); q = np.ascontiguousarray(q, np.float64)
    dI, dO = ctx.to_device(Pin), ctx.to_device(Pout)
    ctx.check(_L().lvk_ekf_cov_propagate_augment(ctx.h, _p(dI), Pin.shape[1], _p(dO), Pout.shape[1], int(n_out), int(pose_rows), phi.shape[0], _p(phi), _p(q)))
    return ctx.to_host(dO, np.float64, Pout.shape)


def cov_gather(ctx, Pin, Pout, idx):
    Pin = np.ascontiguousarray(Pin, np.float64); Pout = np.ascontiguousarray(Pout, np.float64); idx = np.ascontiguousarray(idx, np.int32)
    dI, dO = ctx.to_device(Pin), ctx.to_device(Pout)
    ctx.check(_L().lvk_ekf_cov_gather(ctx.h, _p(dI), Pin.shape[1], _p(dO), Pout.shape[1], _p(idx), len(idx)))
    return ctx.to_host(dO, np.float64, Pout.shape)


def cov_reanchor(ctx, P, n, J, fc):
    P = np.ascontiguousarray(P, np.float64); J = np.ascontiguousarray(J, np.float64)
    dP = ctx.to_device(P)
    ctx.check(_L().lvk_ekf_cov_reanchor(ctx.h, _p(dP), P.shape[1], int(n), _p(J), int(fc)))
    return ctx.to_host(dP, np.float64, P.shape)


def cov_append_features(ctx, P, n, H1, H2, r1, dx, sigma2):
    """-> (P buffer, dx_new).  H1: nn x ldh buffer; H2, r1: nn; dx: n."""
    P = np.ascontiguousarray(P, np.float64); H1 = np.ascontiguousarray(H1, np.float64)
    H2 = np.ascontiguousarray(H2, np.float64); r1 = np.ascontiguousarray(r1, np.float64); dx = np.ascontiguousarray(dx, np.float64)
    nn = len(H2)
    dP, dH1, dr1, ddx, dxn = ctx.to_device(P), ctx.to_device(H1), ctx.to_device(r1), ctx.to_device(dx), ctx.alloc(8 * max(nn, 1))
    ctx.check(_L().lvk_ekf_cov_append_features(ctx.h, _p(dP), P.shape[1], int(n), nn, _p(dH1), H1.shape[1], _p(H2), _p(dr1), _p(ddx), float(sigma2), _p(dxn)))
    return ctx.to_host(dP, np.float64, P.shape), ctx.to_host(dxn, np.float64, (nn,))


def _padded_qr(H, r, ld):
    """[H | r] as the filter hands it to a compression: H with leading dimension ld in a buffer of rows + 2 rows, r in one of rows + 2
    entries, NaN everywhere outside"""
    return _padded(H, ld, H.shape[0] + 2), np.concatenate([r, np.full(2, np.nan)])


def compress_qr(ctx, H, r, ld=None):
    """lvk_ekf_compress_qr on host arrays -> (H', r').  ld: the buffers of _padded_qr; the whole buffers are then returned with the
    number of rows the call left: (H buffer, r buffer, rows_out)."""
    H = np.array(H, np.float64, order="C"); r = np.array(r, np.float64)
    rows, cols = H.shape
    if ld is not None:
        H, r = _padded_qr(H, r, ld)
    dH, dr = ctx.to_device(H), ctx.to_device(r)
    out = C.c_int(0)
    ctx.check(_L().lvk_ekf_compress_qr(ctx.h, _p(dH), H.shape[1], rows, cols, _p(dr), C.byref(out)))
    k = out.value
    if ld is not None:
        return ctx.to_host(dH, np.float64, H.shape), ctx.to_host(dr, np.float64, r.shape), k
    return ctx.to_host(dH, np.float64, (rows, cols))[:k].copy(), ctx.to_host(dr, np.float64, (rows,))[:k].copy()


def _group_arrays(groups):
    rows = np.ascontiguousarray([g[0] for g in groups], np.int32)
    off = np.zeros(len(groups) + 1, np.int32)
    for k, g in enumerate(groups):
        off[k + 1] = off[k] + len(g[1])
    cols = np.ascontiguousarray(np.concatenate([np.asarray(g[1], np.int32) for g in groups]) if groups else np.zeros(0, np.int32), np.int32)
    return rows, off, cols


def qr_plan(N, groups):
    """lvk_ekf_qr_plan (host only): groups = [(rows, ascending column list), ...] in stacking order ->
    (levels, final_rows), levels = [dict(blocks=[dict(in_start, in_rows, out_start, out_rows, ncols, col_off, copy)], cols=int array)]"""
    rows, off, cols = _group_arrays(groups)
    cap_b, cap_c, cap_l = 4 * len(groups) + 16, 8 * (len(cols) + 16), 16
    blocks = np.zeros((cap_b, 8), np.int32); bcols = np.zeros(cap_c, np.int32); lb = np.zeros(cap_l, np.int32); lc = np.zeros(cap_l, np.int32)
    fin = C.c_int(0)
    n = _L().lvk_ekf_qr_plan(int(N), len(groups), _p(rows), _p(off), _p(cols), _p(blocks), cap_b, _p(bcols), cap_c, _p(lb), _p(lc), cap_l, C.byref(fin))
    if n < 0:
        raise LvkError("lvk_ekf_qr_plan failed")
    levels = []; ob = oc = 0
    keys = ("in_start", "in_rows", "out_start", "out_rows", "ncols", "col_off", "copy")
    for l in range(n):
        levels.append(dict(blocks=[dict(zip(keys, map(int, b[:7]))) for b in blocks[ob:ob + lb[l]]], cols=bcols[oc:oc + lc[l]].copy()))
        ob += lb[l]; oc += lc[l]
    return levels, fin.value


def compress_qr_groups(ctx, H, r, groups, ld=None):
    """lvk_ekf_compress_qr_groups on host arrays: H (rows x cols), r, groups = [(rows, ascending column list), ...] -> (H', r').
    ld: as compress_qr."""
    H = np.ascontiguousarray(H, np.float64); r = np.ascontiguousarray(r, np.float64)
    rows, cols = H.shape
    if ld is not None:
        H, r = _padded_qr(H, r, ld)
    gr, off, gc = _group_arrays(groups)
    dH = ctx.to_device(H); dr = ctx.to_device(r)
    out = C.c_int(0)
    ctx.check(_L().lvk_ekf_compress_qr_groups(ctx.h, _p(dH), H.shape[1], rows, cols, _p(dr), len(groups), _p(gr), _p(off), _p(gc), C.byref(out)))
    k = out.value
    if ld is not None:
        return ctx.to_host(dH, np.float64, H.shape), ctx.to_host(dr, np.float64, r.shape), k
    return ctx.to_host(dH, np.float64, (rows, cols))[:k].copy(), ctx.to_host(dr, np.float64, (rows,))[:k].copy()


def make_ekf_config(config):
    """lvk_ekf_config from the dict of LarVio parameters (larvio_amd.synthetic.backend_config)"""
    c = EkfConfig()
    for k in _CFG_INT + _CFG_DBL:
        setattr(c, k, config[k])
    c.intrinsics = (C.c_double * 4)(*config["intrinsics"])
    c.T_cam_imu = (C.c_double * 16)(*np.asarray(config["T_cam_imu"], np.float64).reshape(16))
    c.feature_idp_dim = config.get("feature_idp_dim", 1); c.use_schmidt = config.get("use_schmidt", 0)
    c.calib_imu_instrinsic = config.get("calib_imu_instrinsic", 0); c.max_features = config.get("max_features", 0)
    c.legacy_grid = config.get("legacy_grid", 0)          # 0 = the reference's grid_map bookkeeping (lvk_c.h)
    return c


class LarVio:
    def __init__(self, config, ctx=None):
        """config: dict with the keys LarVio::loadParameters reads (larvio.cpp:58-311; see synthetic.backend_config), or the path
        of a LARVIO configuration file (the reference's constructor argument)."""
        if isinstance(config, (str, os.PathLike)):
            from .config import load_config
            config = load_config(config)[1]
        self.config = dict(config)
        self.ctx = ctx
        self._h = None

    def initialize(self):
        if self.ctx is None:
            self.ctx = Context()
        c = make_ekf_config(self.config)
        h = C.c_void_p()
        st = _L().lvk_ekf_create(self.ctx.h, C.byref(c), C.byref(h))
        if st != 0:
            print("lvk_ekf_create failed:", lib().lvk_last_error(self.ctx.h).decode())
            return False
        self._h = h
        self.ctx.adopt(self)
        return True

    def processFeatures(self, msg, imu_msg_buffer):
        """msg: MonoCameraMeasurement (or (ts, features)); imu_msg_buffer: structured IMU array.
        Returns (bool, remaining_imu_buffer) — the reference mutates the caller's vector in place."""
        ts, feats = (msg.timeStampToSec, msg.features) if hasattr(msg, "features") else msg
        feats = np.ascontiguousarray(feats, OBS); imu = np.ascontiguousarray(imu_msg_buffer, IMU)
        used, upd = C.c_int(0), C.c_int(0)
        self.ctx.check(_L().lvk_ekf_process(self._h, float(ts), _p(feats), len(feats), _p(imu), len(imu), C.byref(used), C.byref(upd)))
        return bool(upd.value), imu[used.value:]

    def processFeaturesAsync(self, msg, imu_msg_buffer):
        """lvk_ekf_process_async: same arguments and return value as processFeatures, but the update itself runs on the filter's
        worker thread and stream; any getter (or the next update, or wait()) waits for it."""
        ts, feats = (msg.timeStampToSec, msg.features) if hasattr(msg, "features") else msg
        feats = np.ascontiguousarray(feats, OBS); imu = np.ascontiguousarray(imu_msg_buffer, IMU)
        used, upd = C.c_int(0), C.c_int(0)
        L = _L()
        L.lvk_ekf_process_async.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]; L.lvk_ekf_process_async.restype = C.c_int
        self.ctx.check(L.lvk_ekf_process_async(self._h, float(ts), _p(feats), len(feats), _p(imu), len(imu), C.byref(used), C.byref(upd)))
        return bool(upd.value), imu[used.value:]

    def wait(self):
        """lvk_ekf_wait: block until the deferred update is done; raises if it failed; -> whether it updated"""
        L = _L()
        L.lvk_ekf_wait.argtypes = [C.c_void_p, C.c_void_p]; L.lvk_ekf_wait.restype = C.c_int
        upd = C.c_int(0)
        self.ctx.check(L.lvk_ekf_wait(self._h, C.byref(upd)))
        return bool(upd.value)

    def set_state(self, t, q, p, v, bg, ba, gyro_old, acc_old):
        a = [np.ascontiguousarray(x, np.float64) for x in (q, p, v, bg, ba, gyro_old, acc_old)]
        self.ctx.check(_L().lvk_ekf_set_state(self._h, float(t), *[_p(x) for x in a]))

    @property
    def dim(self):
        return _L().lvk_ekf_dim(self._h)

    @property
    def initialized(self):
        return bool(_L().lvk_ekf_is_initialized(self._h))

    @property
    def take_off_stamp(self):
        """larvio.cpp:380 — state time at which the initializer succeeded"""
        return float(_L().lvk_ekf_take_off_stamp(self._h))

    def state(self):
        o = np.zeros(30); self.ctx.check(_L().lvk_ekf_get_state(self._h, _p(o)))
        return dict(t=o[0], q=o[1:5].copy(), v=o[5:8].copy(), p=o[8:11].copy(), bg=o[11:14].copy(), ba=o[14:17].copy(),
                    R_b2c=o[17:26].reshape(3, 3).copy(), t_c_b=o[26:29].copy(), td=o[29])

    def stable_map_points(self):
        """getStableMapPointPositions (larvio.cpp:2717-2722): (ids, positions) of in-state features lost since the last call"""
        ids = np.zeros(4096, np.int64); pos = np.zeros((4096, 3))
        n = _L().lvk_ekf_take_lost_features(self._h, _p(ids), _p(pos), 4096)
        return ids[:n].copy(), pos[:n].copy()

    def get_feature_cov(self):
        """lvk_ekf_get_feature_cov: (ids, anchor clone ids, world positions, Sigma (n, 3, 3)) of the in-state features, in the order of
        features(); Sigma is all NaN for a feature whose anchor clone has left the window"""
        cap = 4096
        ids = np.zeros(cap, np.int64); anc = np.zeros(cap, np.int64); pos = np.zeros((cap, 3)); cov = np.zeros((cap, 3, 3)); n = C.c_int(0)
        self.ctx.check(_L().lvk_ekf_get_feature_cov(self._h, _p(ids), _p(anc), _p(pos), _p(cov), cap, C.byref(n)))
        n = n.value
        return ids[:n].copy(), anc[:n].copy(), pos[:n].copy(), cov[:n].copy()

    def get_features_in_camera(self, to_clone_id=-1):
        """lvk_ekf_get_feature_rel: (ids, anchor clone ids, positions (n, 3) in the camera frame of the target pose, Sigma (n, 3, 3)
        there) of the in-state features, in the order of features().  to_clone_id -1: the current IMU state; otherwise the id of a clone
        of clones() (an id outside the window raises LvkError, the filter stays usable).  Position and Sigma are all NaN for a feature
        whose anchor clone has left the window.  The depth sigma of point k is sqrt(Sigma[k, 2, 2])."""
        cap = 4096
        ids = np.zeros(cap, np.int64); anc = np.zeros(cap, np.int64); pos = np.zeros((cap, 3)); cov = np.zeros((cap, 3, 3)); n = C.c_int(0)
        self.ctx.check(_L().lvk_ekf_get_feature_rel(self._h, int(to_clone_id), _p(ids), _p(anc), _p(pos), _p(cov), cap, C.byref(n)))
        n = n.value
        return ids[:n].copy(), anc[:n].copy(), pos[:n].copy(), cov[:n].copy()

    def set_lost_feature_cov(self, on=True):
        """lvk_ekf_set_lost_feature_cov: while on, every in-state feature that is lost gets its position covariance computed before its
        column leaves the covariance (take_lost_features_cov hands it out)"""
        self.ctx.check(_L().lvk_ekf_set_lost_feature_cov(self._h, int(bool(on))))

    def take_lost_features_cov(self):
        """lvk_ekf_take_lost_features_cov: stable_map_points() with each point's Sigma: (ids, positions, Sigma (n, 3, 3)); NaN
        matrices for points queued while the switch was off"""
        ids = np.zeros(4096, np.int64); pos = np.zeros((4096, 3)); cov = np.zeros((4096, 3, 3))
        n = _L().lvk_ekf_take_lost_features_cov(self._h, _p(ids), _p(pos), _p(cov), 4096)
        return ids[:n].copy(), pos[:n].copy(), cov[:n].copy()

    def set_msckf_points(self, on=True):
        """lvk_ekf_set_msckf_points: while on, every MSCKF feature a lost-feature update triangulates, accepts and erases is kept with
        its position covariance (take_msckf_points hands it out); refused (LvkError) with a shard transport set"""
        self.ctx.check(_L().lvk_ekf_set_msckf_points(self._h, int(bool(on))))

    def take_msckf_points(self):
        """lvk_ekf_take_msckf_points: (ids, world positions, Sigma (n, 3, 3), observation counts) of the MSCKF points collected since
        the last call; Sigma is stated against the covariance before the update that consumed the point (conservative)"""
        out = [[], [], [], []]
        while True:
            ids = np.zeros(4096, np.int64); pos = np.zeros((4096, 3)); cov = np.zeros((4096, 3, 3)); nob = np.zeros(4096, np.int32)
            n = _L().lvk_ekf_take_msckf_points(self._h, _p(ids), _p(pos), _p(cov), _p(nob), 4096)
            for o, a in zip(out, (ids, pos, cov, nob)):
                o.append(a[:n].copy())
            if n < 4096:
                break
        return tuple(np.concatenate(o) for o in out)

    def set_keyframe_export(self, on=True):
        """lvk_ekf_set_keyframe_export: while on, every clone the pruning removes is kept as a KEYFRAME record with its absolute 6 x 6
        covariance and the covariance of its pose relative to the nearest newer surviving clone (take_keyframes hands them out);
        refused (LvkError) with a shard transport set"""
        self.ctx.check(_L().lvk_ekf_set_keyframe_export(self._h, int(bool(on))))

    def take_keyframes(self):
        """lvk_ekf_take_keyframes: a structured array (dtype KEYFRAME) of the clones pruned since the last call, in pruning order"""
        out = []
        while True:
            buf = np.zeros(1024, KEYFRAME)
            n = _L().lvk_ekf_take_keyframes(self._h, _p(buf), 1024)
            out.append(buf[:n].copy())
            if n < 1024:
                break
        return np.concatenate(out)

    def get_window_cov(self):
        """lvk_ekf_get_window_cov: (ids, absolute blocks (n, 6, 6), Sigma_rel of clone i to clone i + 1 (n, 6, 6); NaN for the last clone)
        for the clones of clones(), in that order"""
        cap = 256
        ids = np.zeros(cap, np.int64); ca = np.zeros((cap, 6, 6)); cr = np.zeros((cap, 6, 6)); n = C.c_int(0)
        self.ctx.check(_L().lvk_ekf_get_window_cov(self._h, _p(ids), _p(ca), _p(cr), cap, C.byref(n)))
        n = n.value
        return ids[:n].copy(), ca[:n].copy(), cr[:n].copy()

    def add_fix(self, p, cov, time=0.0, clone_id=-1, q=None, lever=(0.0, 0.0, 0.0), tag=0):
        """lvk_ekf_add_fix: queue an external fix, expressed in the filter's world frame, on the clone `clone_id` or (clone_id -1) on the
        clone at `time` (IMU clock, as clones()["time"]).  q None: a POSITION fix, p the position of the point at `lever` (body frame),
        cov its 3 x 3 covariance; with q ([x y z w], body to world): a POSE fix, cov 6 x 6 in the order [d_theta; p].  Applied by the next
        update that holds the clone; take_fix_reports() says what became of it.  Raises LvkError for what the header lists as refused."""
        f = np.zeros(1, FIX)
        cov = np.asarray(cov, np.float64); m = 3 if q is None else 6
        if cov.shape != (m, m):
            raise ValueError("add_fix: cov must be %d x %d" % (m, m))
        f["tag"] = tag; f["kind"] = FIX_POSITION if q is None else FIX_POSE; f["clone_id"] = clone_id; f["time"] = time
        f["p"] = p; f["lever"] = lever; f["q"] = (0, 0, 0, 1) if q is None else q; f["cov"][0, :m, :m] = cov
        self.ctx.check(_L().lvk_ekf_add_fix(self._h, _p(f)))

    def set_fix_options(self, gate_scale=1.0, max_gap_s=0.0):
        """lvk_ekf_set_fix_options: the gate of a fix is gate_scale times the filter's own chi-square table entry (<= 0: no gate);
        max_gap_s: a POSITION fix between two adjacent clones at most this far apart is interpolated (0: never)"""
        self.ctx.check(_L().lvk_ekf_set_fix_options(self._h, float(gate_scale), float(max_gap_s)))

    def take_fix_reports(self):
        """lvk_ekf_take_fix_reports: a structured array (dtype FIX_REPORT), one record per fix consumed since the last call, in order"""
        out = []
        while True:
            buf = np.zeros(256, FIX_REPORT)
            n = _L().lvk_ekf_take_fix_reports(self._h, _p(buf), 256)
            out.append(buf[:n].copy())
            if n < 256:
                break
        return np.concatenate(out)

    def fix_stats(self):
        o = np.zeros(8, np.int64); _L().lvk_ekf_fix_stats(self._h, _p(o))
        return dict(queued=int(o[0]), applied=int(o[1]), gated=int(o[2]), not_pd=int(o[3]), stale=int(o[4]), no_clone=int(o[5]), waiting=int(o[6]),
                    interpolated=int(o[7]))

    def add_landmark_obs(self, p_w, uv, sigma, cov_w=None, time=0.0, clone_id=-1, tag=0):
        """lvk_ekf_add_landmark_obs: queue one batch - the observations uv (k x 2, normalised image coordinates, standard deviation sigma:
        a number or k of them) made in ONE image of the known world points p_w (k x 3, the filter's world frame; cov_w: None, one 3 x 3
        or k of them) - on the clone `clone_id` or (clone_id -1) on the clone at `time`.  Applied by the next update that holds the clone;
        take_landmark_reports() says what became of it.  Raises LvkError for what the header lists as refused."""
        p_w = np.asarray(p_w, np.float64).reshape(-1, 3); k = len(p_w)
        from .ops import LANDMARK_OBS
        o = np.zeros(k, LANDMARK_OBS)
        o["p_w"] = p_w; o["uv"] = np.asarray(uv, np.float64).reshape(k, 2); o["sigma"] = sigma
        if cov_w is not None:
            o["cov_w"] = np.asarray(cov_w, np.float64).reshape(-1, 9)
        self.ctx.check(_L().lvk_ekf_add_landmark_obs(self._h, int(tag), int(clone_id), float(time), _p(o) if k else None, k))

    def set_landmark_options(self, gate_scale=1.0, min_depth=0.1):
        """lvk_ekf_set_landmark_options: the gate of one observation is gate_scale times the filter's own chi-square table entry for 2
        degrees of freedom (<= 0: no gate); an observation whose depth in the camera is <= min_depth counts as behind"""
        self.ctx.check(_L().lvk_ekf_set_landmark_options(self._h, float(gate_scale), float(min_depth)))

    def take_landmark_reports(self):
        """lvk_ekf_take_landmark_reports: a structured array (dtype LANDMARK_REPORT), one record per batch consumed since the last call"""
        out = []
        while True:
            buf = np.zeros(64, LANDMARK_REPORT)
            n = _L().lvk_ekf_take_landmark_reports(self._h, _p(buf), 64)
            out.append(buf[:n].copy())
            if n < 64:
                break
        return np.concatenate(out)

    def landmark_stats(self):
        o = np.zeros(12, np.int64); _L().lvk_ekf_landmark_stats(self._h, _p(o))
        return dict(queued=int(o[0]), applied=int(o[1]), all_rejected=int(o[2]), not_pd=int(o[3]), stale=int(o[4]), no_clone=int(o[5]), waiting=int(o[6]),
                    obs=int(o[7]), used=int(o[8]), gated=int(o[9]), behind=int(o[10]))

    def set_shard(self, rank, world, fn, user, keepalive=None):
        """lvk_ekf_set_shard: this filter does the per-feature device work of rank `rank` of `world`; fn/user = the all-gather
        (larvio_amd.sharding.RcclShard(...).args() or HostExchange(...).args())."""
        self._shard_keep = keepalive
        self.ctx.check(_L().lvk_ekf_set_shard(self._h, int(rank), int(world), fn, user))

    def shard_stats(self):
        o = np.zeros(8, np.int64); _L().lvk_ekf_shard_stats(self._h, _p(o))
        return dict(exchanges=int(o[0]), bytes_sent=int(o[1]), sharded_updates=int(o[2]), rows_stacked=int(o[3]),
                    qr_updates=int(o[4]), qr_levels=int(o[5]), qr_rows_in=int(o[6]), qr_rows_out=int(o[7]))

    def profile(self, enable=True):
        """HIP-event time of the H P GEMM since the last call: dict(ms, flops, launches); enables/disables the bracket"""
        o = np.zeros(3); self.ctx.check(_L().lvk_ekf_profile(self._h, int(enable), _p(o)))
        return dict(ms=o[0], flops=o[1], launches=int(o[2]))

    def profile_qr(self):
        """HIP-event time of the structure-aware TSQR levels (k_qr_sparse) since the last call, while profile(True) is on:
        dict(ms, flops on the structure factored, launches, rows entering the levels)"""
        L = _L(); L.lvk_ekf_profile_qr.argtypes = [C.c_void_p, C.c_void_p]; L.lvk_ekf_profile_qr.restype = C.c_int
        o = np.zeros(4); self.ctx.check(L.lvk_ekf_profile_qr(self._h, _p(o)))
        return dict(ms=o[0], flops=o[1], launches=int(o[2]), rows=o[3])

    def imu_intrinsics(self):
        """T1 T2 T3 A1 A2 A3 M1 M2 (24 numbers; state columns 22..45 when calib_imu_instrinsic = 1)"""
        o = np.zeros(24); self.ctx.check(_L().lvk_ekf_get_imu_intrinsics(self._h, _p(o))); return o

    def set_imu_intrinsics(self, v):
        v = np.ascontiguousarray(v, np.float64); assert v.shape == (24,)
        self.ctx.check(_L().lvk_ekf_set_imu_intrinsics(self._h, _p(v)))

    def cov(self):
        N = self.dim; P = np.zeros((N, N)); self.ctx.check(_L().lvk_ekf_get_cov(self._h, _p(P))); return P

    def set_cov(self, P):
        """lvk_ekf_set_cov: replace the covariance (dim x dim); refused while a deferred update is in flight"""
        P = np.ascontiguousarray(P, np.float64)
        if P.ndim != 2 or P.shape[0] != P.shape[1]:
            raise ValueError("set_cov: a square matrix is expected")
        self.ctx.check(_L().lvk_ekf_set_cov(self._h, _p(P), P.shape[0]))

    def set_indefinite_policy(self, policy):
        """lvk_ekf_set_indefinite_policy: INDEFINITE_FAIL (0, the default: LVK_ERR_NUMERIC, the handle stays failed) or INDEFINITE_LDLT
        (1: that update runs again through the pivoted LDL^T, as the reference does, and the filter goes on)"""
        self.ctx.check(_L().lvk_ekf_set_indefinite_policy(self._h, int(policy)))

    def last_update(self):
        """lvk_ekf_last_update: (H, r, P, state30) - the stacked system the most recent update read, with covariance and state as they
        are now; also on a handle that failed with LVK_ERR_NUMERIC (then: what that update started from)"""
        m, n = C.c_int(0), C.c_int(0)
        self.ctx.check(_L().lvk_ekf_last_update(self._h, C.byref(m), C.byref(n), None, None, None, None))
        H = np.zeros((m.value, n.value)); r = np.zeros(m.value); P = np.zeros((n.value, n.value)); s = np.zeros(30)
        self.ctx.check(_L().lvk_ekf_last_update(self._h, C.byref(m), C.byref(n), _p(H), _p(r), _p(P), _p(s)))
        return H, r, P, s

    def indefinite_fallbacks(self):
        return int(_L().lvk_ekf_indefinite_fallbacks(self._h))

    def cov_imu(self, n=9):
        """the covariance's leading n x n block (n <= 16): what getPpose / getPvel read, served without moving the matrix"""
        P = np.zeros((n, n)); self.ctx.check(_L().lvk_ekf_get_cov_imu(self._h, n, _p(P))); return P

    def clones(self):
        o = np.zeros(256, CLONE); n = _L().lvk_ekf_get_clones(self._h, _p(o), 256); return o[:n].copy()

    def features(self):
        ids = np.zeros(4096, np.int64); idp = np.zeros(4096); pos = np.zeros((4096, 3))
        n = _L().lvk_ekf_get_features(self._h, _p(ids), _p(idp), _p(pos), 4096)
        return ids[:n].copy(), idp[:n].copy(), pos[:n].copy()

    def counters(self):
        o = np.zeros(8, np.int64); _L().lvk_ekf_counters(self._h, _p(o))
        return dict(hybrid=int(o[0]), msckf=int(o[1]), last_rows=int(o[2]), zupt=int(o[3]), gated_in=int(o[4]), gated_out=int(o[5]),
                    map=int(o[6]), triangulations=int(o[7]))

    def init_report(self):
        """lvk_ekf_init_report: what the moving-start initialiser handed to the filter + the successful attempt's intermediate results
        (None until it has succeeded on this handle)"""
        r = InitReport(); rc = _L().lvk_ekf_init_report(self._h, C.byref(r))
        if rc != 0:
            raise LvkError("lvk_ekf_init_report failed (%d)" % rc)
        if not r.valid:
            return None
        a = lambda x, shape=None: np.array(x, np.float64).reshape(shape) if shape else np.array(x, np.float64)
        return dict(message=r.message, attempts=r.attempts, ransac_calls=r.ransac_calls, l=r.l, n_points=r.n_points, erase=r.erase, state_time=r.state_time, scale=r.scale,
                    relR=a(r.rel_R, (3, 3)), relT=a(r.rel_T), sfm_R=a(r.sfm_R, (11, 3, 3)), sfm_T=a(r.sfm_T, (11, 3)), bg=a(r.bg), g=a(r.g), q=a(r.q), v=a(r.v))

    # reference getters (larvio.cpp:2644-2735)
    def getTbw(self):
        s = self.state(); q = s["q"]
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4); T[:3, :3] = R; T[:3, 3] = s["p"]
        return T

    def getVel(self):
        return self.state()["v"]

    def close(self):
        if self._h:
            _L().lvk_ekf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
