"""ImageProcessor — host-side mirror of larvio::ImageProcessor over the C ABI.

Same surface as the reference class (include/larvio/image_processor.h:36-68): construct with the
configuration, ``initialize()``, then ``processImage(img, imu_buffer)`` per frame; the boolean it returns is
the reference's ``haveFeatures`` and the feature list is the ``MonoCameraMeasurement`` it fills
(include/larvio/feature_msg.h:15-52).  All arithmetic happens in liblvk_hip.so on the GPU.
"""
import ctypes as C
import os
import numpy as np
from ._lib import lib, _p, Context, FeConfig, LvkError, IMU, OBS, make_image, PIX_FORMATS


class MonoCameraMeasurement:
    """feature_msg.h:47-52"""

    def __init__(self, time_stamp, features):
        self.timeStampToSec = time_stamp
        self.features = features          # structured array, dtype OBS (id,u,v,u_init,v_init,u_vel,v_vel,u_init_vel,v_init_vel)


def make_fe_config(config):
    """lvk_fe_config from the dict of ImageProcessor parameters (larvio_amd.synthetic.frontend_config)"""
    c = FeConfig()
    for k in ("width", "height", "pyramid_levels", "patch_size", "max_iteration", "track_precision",
              "max_features_num", "min_distance", "flag_equalize", "pub_frequency", "distortion_model"):
        setattr(c, k, config[k])
    c.intrinsics = (C.c_double * 4)(*config["intrinsics"])
    c.distortion = (C.c_double * 4)(*config["distortion"])
    c.R_cam_imu = (C.c_double * 9)(*np.asarray(config["R_cam_imu"], np.float64).reshape(9))
    return c


class ImageProcessor:
    FIRST_IMAGE, SECOND_IMAGE, OTHER_IMAGES = 1, 2, 3

    def __init__(self, config, ctx=None):
        """config: dict with the keys ImageProcessor::loadParameters reads (image_processor.cpp:44-113; see
        larvio_amd.synthetic.frontend_config), or the path of a LARVIO configuration file."""
        if isinstance(config, (str, os.PathLike)):          # the reference's constructor argument: the YAML path
            from .config import load_config
            config = load_config(config)[0]
        self.config = dict(config)
        self.ctx = ctx
        self._h = None
        self._pixfmt = "mono8"

    def initialize(self):
        if self.ctx is None:
            self.ctx = Context()
        c = make_fe_config(self.config)
        h = C.c_void_p()
        st = lib().lvk_frontend_create(self.ctx.h, C.byref(c), C.byref(h))
        if st != 0:
            print("lvk_frontend_create failed:", lib().lvk_last_error(self.ctx.h).decode())
            return False
        self._h = h
        self.ctx.adopt(self)
        self._cap = self.config["max_features_num"]
        self._out = np.zeros(self._cap, OBS)
        return True

    def processImage(self, img, imu_msg_buffer, ts=None, device_ptr=None, stride=None, shape=None):
        """img: (H,W) uint8 array (host; its shape is checked against the configured resolution, as a cv::Mat's would be; after
        set_input_format: the array that format demands) — or pass
        device_ptr/stride (and shape=(H,W) if it is not the configured one) for an image already in HBM.
        imu_msg_buffer: structured array (t, gyro[3], acc[3]).  Returns (haveFeatures, MonoCameraMeasurement|None)."""
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        imu = np.ascontiguousarray(imu_msg_buffer, IMU)
        n_out, has = C.c_int(0), C.c_int(0)
        im, keep = make_image(img, device_ptr, stride, shape if shape is not None else (self.config["height"], self.config["width"]), fmt=self._pixfmt)
        st = lib().lvk_frontend_process(self._h, C.byref(im), float(ts), _p(imu), len(imu), _p(self._out), self._cap,
                                        C.byref(n_out), C.byref(has))
        self.ctx.check(st)
        if not has.value:
            return False, None
        return True, MonoCameraMeasurement(float(ts), self._out[:n_out.value].copy())

    # ---- introspection used by the parity tests
    def tracks(self):
        cap = self._cap
        ids = np.empty(cap, np.uint64); p = np.empty((cap, 2), np.float32); life = np.empty(cap, np.int32)
        ini = np.empty((cap, 2), np.float32); desc = np.empty((cap, 32), np.uint8); n = C.c_int(0)
        self.ctx.check(lib().lvk_frontend_tracks(self._h, _p(ids), _p(p), _p(life), _p(ini), _p(desc), cap, C.byref(n)))
        n = n.value
        return dict(ids=ids[:n].copy(), pts=p[:n].copy(), lifetime=life[:n].copy(), init=ini[:n].copy(), desc=desc[:n].copy())

    def new_pts(self):
        p = np.empty((self._cap, 2), np.float32); n = C.c_int(0)
        self.ctx.check(lib().lvk_frontend_new_pts(self._h, _p(p), self._cap, C.byref(n)))
        return p[:n.value].copy()

    def set_mask(self, mask, device_ptr=None, stride=None, shape=None):
        """Region mask for corner detection (lvk_frontend_set_mask; the reference has no such call): non-zero = corners may be
        detected there, None clears.  mask: (H,W) uint8 array of the configured resolution (strided views are passed as they are), or
        a device tensor (anything with data_ptr()) - or pass device_ptr/stride/shape as processImage does.  Holds from the next
        processed frame on; with a VioPipeline call it before the first step or after drain()."""
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        if mask is None and device_ptr is None:
            self.ctx.check(lib().lvk_frontend_set_mask(self._h, None))
            return
        if mask is not None and hasattr(mask, "data_ptr"):
            if mask.dim() != 2 or mask.element_size() != 1 or mask.stride(1) != 1:
                raise ValueError("a device mask must be a 2-D uint8 tensor with unit column stride")
            device_ptr, stride, shape, mask = mask.data_ptr(), mask.stride(0), tuple(mask.shape), None
        im, keep = make_image(mask, device_ptr, stride, shape if shape is not None else (self.config["height"], self.config["width"]))
        self.ctx.check(lib().lvk_frontend_set_mask(self._h, C.byref(im)))

    @property
    def has_mask(self):
        return bool(lib().lvk_frontend_has_mask(self._h))

    def set_input_format(self, fmt, shift=0):
        """Pixel format of every image from now on (lvk_frontend_set_input_format; the reference's ROS caller converts on the host
        instead): "mono8" (the default), "bgr8", "rgb8", "bgra8", "rgba8" - (H, W, 3|4) uint8 -, "mono16" - (H, W) uint16, grey =
        min(255, v >> shift), shift 0..8 -, "yuyv", "uyvy" - (H, W, 2) uint8, grey = Y.  The bytes are uploaded as they are and converted
        on the GPU (include/lvk_c.h states the formulas); a device pointer's stride is in bytes.  With a VioPipeline call it before the
        first step or after drain().  A refusal (LvkError) leaves the previous format in force."""
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        if fmt not in PIX_FORMATS:
            raise ValueError(f"unknown pixel format {fmt!r}: one of {', '.join(PIX_FORMATS)}")
        self.ctx.check(lib().lvk_frontend_set_input_format(self._h, PIX_FORMATS[fmt], int(shift)))
        self._pixfmt = fmt

    @property
    def input_format(self):
        """name of the pixel format in force (lvk_frontend_input_format)"""
        v = lib().lvk_frontend_input_format(self._h)
        return next(k for k, n in PIX_FORMATS.items() if n == v)

    def match_landmarks(self, pred_px, radius, desc, max_candidates=0, quality=0.0, min_distance=0.0, max_dist=0, ratio_pct=0):
        """lvk_frontend_match_landmarks: where in the last processed frame are these map points?  pred_px (n, 2): their predicted pixels
        (larvio_amd.localize.predict_pixels), radius: the search radius in pixels (a number or n of them), desc (n, 32) uint8: their
        descriptors (tracks()["desc"] of the run that mapped them).  Options left at zero take the library's defaults: 4096 candidates,
        quality 0.01, the configured min_distance, max_dist 58, ratio_pct 100 (no ratio test).  -> a structured array (dtype
        LANDMARK_MATCH: status, dist, second, n_window, px, und) of n records - status MATCH_OK (0) marks a match, und is what
        LarVio.add_landmark_obs takes as uv; self.last_match_candidates = the corners the frame offered.  With a VioPipeline call it only
        after drain()."""
        from ._lib import MATCH_QUERY, LANDMARK_MATCH, MatchOptions
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        p = np.ascontiguousarray(np.asarray(pred_px, np.float32).reshape(-1, 2)); n = len(p)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if len(d) != n:
            raise ValueError(f"{n} predicted pixels but {len(d)} descriptors")
        q = np.zeros(n, MATCH_QUERY); q["x"] = p[:, 0]; q["y"] = p[:, 1]; q["radius"] = radius
        out = np.zeros(n, LANDMARK_MATCH); nc = C.c_int(0)
        o = MatchOptions(int(max_candidates), float(quality), float(min_distance), int(max_dist), int(ratio_pct))
        self.ctx.check(lib().lvk_frontend_match_landmarks(self._h, _p(q) if n else None, _p(d) if n else None, n, C.byref(o), _p(out) if n else None, C.byref(nc)))
        self.last_match_candidates = nc.value
        return out

    def align_landmarks(self, matches, R_wc, p_wc, thresh=0.0, min_depth=0.0, min_dz=0.0, min_inliers=0, max_refine_iters=0, max_hypotheses=0, seed=0):
        """lvk_frontend_align_landmarks: the yaw and translation that take a prior map's frame into the filter's world frame, p_w = Rz X + t,
        from putative matches of the map's points in the last processed frame.  matches: an ALIGN_MATCH array (X: the map point, u, v: the
        normalised observation - larvio_amd.localize.align_matches builds it from match_landmarks' records), at most 1024; R_wc, p_wc: the
        camera pose of that frame in the filter's world frame (camera-to-world rotation, camera position).  Options left at zero take the
        library's defaults: thresh 0.01, min_depth 0.1, min_dz 1e-6, min_inliers 6, max_refine_iters 10, 4096 hypotheses, the header's
        seed.  -> (result: one ALIGN_RESULT record - status ALIGN_OK (0) marks success; c, s, t the refined alignment, A the normal
        matrix, rms, iters -, mask: (n,) uint8, the winner's inliers).  larvio_amd.localize.apply_alignment takes the result.  With a
        VioPipeline call it only after drain()."""
        from ._lib import ALIGN_MATCH, ALIGN_RESULT, AlignOptions
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        m = np.ascontiguousarray(matches, ALIGN_MATCH); n = len(m)
        R = np.ascontiguousarray(R_wc, np.float64).reshape(9); p = np.ascontiguousarray(p_wc, np.float64).reshape(3)
        out = np.zeros(1, ALIGN_RESULT); mask = np.zeros(max(n, 1), np.uint8)
        o = AlignOptions(float(thresh), float(min_depth), float(min_dz), int(min_inliers), int(max_refine_iters))
        self.ctx.check(lib().lvk_frontend_align_landmarks(self._h, _p(m) if n else None, n, _p(R), _p(p), C.byref(o), int(max_hypotheses), int(seed) & 0xFFFFFFFF,
                                                          _p(out), _p(mask)))
        return out[0], mask[:n]

    def set_map(self, X_map, cov_map, desc):
        """lvk_frontend_set_map: keep a prior map on the device.  X_map (n, 3): its points in the map's own frame, best first - the order
        is the priority match_map selects by -, cov_map: their covariances (n, 3, 3) or None, desc (n, 32) uint8: their descriptors.  Replaces
        a previous map; an empty X_map (or None) frees it.  With a VioPipeline call it only after drain()."""
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        X = np.zeros((0, 3)) if X_map is None else np.ascontiguousarray(X_map, np.float64).reshape(-1, 3)
        n = len(X)
        cv = None if cov_map is None or n == 0 else np.ascontiguousarray(cov_map, np.float64).reshape(-1, 9)
        d = None if n == 0 else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if n and (len(d) != n or (cv is not None and len(cv) != n)):
            raise ValueError(f"{n} map points but {len(d)} descriptors" + ("" if cv is None else f" and {len(cv)} covariances"))
        self.ctx.check(lib().lvk_frontend_set_map(self._h, _p(X) if n else None, _p(cv), _p(d), n))

    @property
    def map_size(self):
        """points of the map in force (lvk_frontend_map_size); 0: none"""
        return lib().lvk_frontend_map_size(self._h)

    def build_map(self, X, cov, desc, score=None, **options):
        """lvk_frontend_build_map: a session's raw exports into the resident map.  X (n, 3), cov (n, 3, 3) or None, desc (n, 32) uint8 -
        larvio_amd.localize.MapCollector.arrays() gives them -, score (n,) or None (smaller is better; without it the covariance's trace
        is the score); options: max_score, r_dup, dup_max_dist of larvio_amd.ops.map_build_options.  Bad points are culled, of
        near-duplicates the better copy is kept, the rest is sorted best first and becomes the map in force exactly as set_map would
        make it (map_size = n_kept).  -> (order: the original indices of the kept points in the map's order - X[order], cov[order],
        desc[order] is the resident map -, info: one MAP_BUILD_INFO record).  A refusal (LvkError) leaves the previous map in place.  With
        a VioPipeline call it only after drain()."""
        from ._lib import MAP_BUILD_INFO
        from .ops import map_build_options
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        Xa = np.zeros((0, 3)) if X is None else np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        n = len(Xa)
        cv = None if cov is None or n == 0 else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
        d = None if n == 0 else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        sc = None if score is None or n == 0 else np.ascontiguousarray(score, np.float64).reshape(-1)
        if n and (len(d) != n or (cv is not None and len(cv) != n) or (sc is not None and len(sc) != n)):
            raise ValueError(f"{n} map points but {len(d)} descriptors" + ("" if cv is None else f", {len(cv)} covariances") + ("" if sc is None else f", {len(sc)} scores"))
        o = map_build_options(**options)
        order = np.zeros(max(n, 1), np.int32); info = np.zeros(1, MAP_BUILD_INFO)
        self.ctx.check(lib().lvk_frontend_build_map(self._h, _p(Xa) if n else None, _p(cv), _p(d), _p(sc), n, C.byref(o), _p(order), n, _p(info)))
        return order[:int(info[0]["n_kept"])].copy(), info[0]

    def match_map(self, R_wc, p_wc, align=None, cov_cam=None, select=None, max_candidates=0, quality=0.0, min_distance=0.0, max_dist=0, ratio_pct=0):
        """lvk_frontend_match_map: the resident map's points in the last processed frame.  R_wc, p_wc: the predicted camera pose in the
        filter's world frame; align: the map's alignment - None (the map is in the world frame), the ALIGN_RESULT record of
        align_landmarks, or (c, s, t); cov_cam: None or the 6 x 6 covariance of that pose in the order [dtheta (camera side), dp (world)];
        select: larvio_amd.ops.map_select_options(...) or None; the rest are match_landmarks' options.  -> (records: a MAP_MATCH array -
        index into the map, cell, q: the query the matcher was given, depth, m: the LANDMARK_MATCH record -, info: one MAP_INFO record).
        larvio_amd.localize.map_obs turns the OK records into observations.  With a VioPipeline call it only after drain()."""
        from ._lib import MAP_MATCH, MAP_INFO, MAP_MAX_QUERIES, MatchOptions
        from .ops import align_record
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        R = np.ascontiguousarray(R_wc, np.float64).reshape(9); p = np.ascontiguousarray(p_wc, np.float64).reshape(3)
        cc = None if cov_cam is None else np.ascontiguousarray(cov_cam, np.float64).reshape(36)
        al = align_record(align)
        out = np.zeros(MAP_MAX_QUERIES, MAP_MATCH); info = np.zeros(1, MAP_INFO); n = C.c_int(0)
        o = MatchOptions(int(max_candidates), float(quality), float(min_distance), int(max_dist), int(ratio_pct))
        self.ctx.check(lib().lvk_frontend_match_map(self._h, _p(al), _p(R), _p(p), _p(cc), C.byref(select) if select is not None else None, C.byref(o), _p(out),
                                                    len(out), C.byref(n), _p(info)))
        return out[:n.value].copy(), info[0]

    def relocalise_map(self, R_wc, p_wc, *, max_matches=0, max_hypotheses=0, seed=0, max_candidates=0, quality=0.0, min_distance=0.0, max_dist=0, ratio_pct=0,
                       thresh=0.0, min_depth=0.0, min_dz=0.0, min_inliers=0, max_refine_iters=0):
        """lvk_frontend_relocalise_map: the yaw and translation of the resident map (set_map) from the last processed frame, in one call and
        whatever the map's size: the frame's corners are searched in the whole map (lvk_orb_match_global), the best max_matches (0 = 1024) OK
        matches in (distance, corner) order go to the two-point RANSAC.  R_wc, p_wc: the camera pose of that frame in the filter's world
        frame; the options are match_landmarks' (ratio_pct=80 is recommended here; the default stays 100, no ratio test) and
        align_landmarks'.  -> (result: one ALIGN_RESULT record, matches: a RELOC_MATCH array - cand: the corner, index: the map point, dist,
        second, px, und, inlier -, info: one GLOBAL_INFO record).  larvio_amd.localize.apply_alignment takes the result, match_map takes it as
        align.  self.last_match_candidates is not touched.  With a VioPipeline call it only after drain()."""
        from ._lib import ALIGN_RESULT, RELOC_MATCH, GLOBAL_INFO, GLOBAL_MAX_MATCHES, MatchOptions, AlignOptions
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        R = np.ascontiguousarray(R_wc, np.float64).reshape(9); p = np.ascontiguousarray(p_wc, np.float64).reshape(3)
        res = np.zeros(1, ALIGN_RESULT); out = np.zeros(GLOBAL_MAX_MATCHES, RELOC_MATCH); info = np.zeros(1, GLOBAL_INFO); n = C.c_int(0)
        mo = MatchOptions(int(max_candidates), float(quality), float(min_distance), int(max_dist), int(ratio_pct))
        ao = AlignOptions(float(thresh), float(min_depth), float(min_dz), int(min_inliers), int(max_refine_iters))
        self.ctx.check(lib().lvk_frontend_relocalise_map(self._h, _p(R), _p(p), C.byref(mo), C.byref(ao), int(max_matches), int(max_hypotheses), int(seed) & 0xFFFFFFFF,
                                                         _p(res), _p(out), len(out), C.byref(n), _p(info)))
        return res[0], out[:n.value].copy(), info[0]

    def merge_map(self, X, cov, desc, align=None, cov_align=None, *, max_hypotheses=0, seed=0, max_dist=0, ratio_pct=0, thresh=0.0, min_rho=0.0, min_inliers=0,
                  **build_options):
        """lvk_frontend_merge_map: a second session's exports merged into the resident map (multi-session mapping).  X (n, 3), cov
        (n, 3, 3), desc (n, 32) uint8: session B in its own world frame; align: B -> the map's frame - None (find it: the sorted B is
        searched in the resident map and lvk_align_ransac_3d aligns the matched points), an ALIGN_RESULT record or (c, s, t);
        larvio_amd.localize.invert_alignment turns the alignment of a session that was localised online; cov_align: None or the 4 x 4
        covariance of the alignment's (psi, t).  max_dist, ratio_pct: the search's; thresh, min_rho, min_inliers: the 3D alignment's (zero =
        0.10 m, 0.5 m, 6); build_options: max_score, r_dup, dup_max_dist of larvio_amd.ops.map_build_options, applied to B alone and to the
        merged map.  -> (align: the ALIGN_RESULT record that was used - with a status other than ALIGN_OK nothing was merged and the map
        in force stands -, order: the merged map's points in the caller's view - a value below the old map_size is that resident point,
        any other is the old map_size + B's original index -, info: one MAP_BUILD_INFO record, match_info: one GLOBAL_INFO record).  A
        refusal (LvkError) leaves the previous map in place.  With a VioPipeline call it only after drain()."""
        from ._lib import ALIGN_RESULT, MAP_BUILD_INFO, GLOBAL_INFO, MatchOptions
        from .ops import map_build_options, align3d_options, align_record
        if self._h is None:
            raise LvkError("ImageProcessor.initialize() has not succeeded")
        Xa = np.zeros((0, 3)) if X is None else np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        n = len(Xa)
        cv = None if cov is None or n == 0 else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
        d = None if desc is None or n == 0 else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        if n and ((d is not None and len(d) != n) or (cv is not None and len(cv) != n)):
            raise ValueError(f"{n} points but {0 if d is None else len(d)} descriptors and {0 if cv is None else len(cv)} covariances")
        al = align_record(align)
        P = None if cov_align is None else np.ascontiguousarray(cov_align, np.float64).reshape(16)
        mo = MatchOptions(0, 0.0, 0.0, int(max_dist), int(ratio_pct)); ao = align3d_options(thresh, min_rho, min_inliers); bo = map_build_options(**build_options)
        cap = max(self.map_size, 0) + n
        used = np.zeros(1, ALIGN_RESULT); order = np.zeros(max(cap, 1), np.int32); info = np.zeros(1, MAP_BUILD_INFO); ginfo = np.zeros(1, GLOBAL_INFO)
        self.ctx.check(lib().lvk_frontend_merge_map(self._h, _p(Xa) if n else None, _p(cv), _p(d), n, _p(al), _p(P), C.byref(mo), C.byref(ao), int(max_hypotheses),
                                                    int(seed) & 0xFFFFFFFF, C.byref(bo), _p(used), _p(order), cap, _p(info), _p(ginfo)))
        return used[0], order[:int(info[0]["n_kept"])].copy(), info[0], ginfo[0]      # (info is zero when nothing was merged)

    @property
    def state(self):
        return lib().lvk_frontend_state(self._h)

    def lk_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(lib().lvk_frontend_lk_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def msg_stats(self):
        """-> (messages published, features they carried in total) since the front-end was created"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx.check(lib().lvk_frontend_msg_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def profile_enable(self, stage_mask=0x1FF):
        self.ctx.check(lib().lvk_frontend_profile_enable(self._h, stage_mask))

    def profile_read(self, reset=True):
        """-> {stage_name: (gpu_ms_sum, launches)} from HIP events on the context stream"""
        from ._lib import FE_STAGES
        ms = np.zeros(FE_STAGES, np.float64); n = np.zeros(FE_STAGES, np.uint64)
        self.ctx.check(lib().lvk_frontend_profile_read(self._h, _p(ms), _p(n), 1 if reset else 0))
        return {lib().lvk_frontend_stage_name(i).decode(): (float(ms[i]), int(n[i])) for i in range(FE_STAGES)}

    def close(self):
        if self._h:
            lib().lvk_frontend_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
