"""Stage-level host wrappers over the C ABI (numpy in / numpy out; data staged through HBM).

These mirror, call for call, the OpenCV / ORBdescriptor functions the reference's front-end invokes
(see include/lvk_c.h for the file:line of each), so the parity tests read like the reference's code.
"""
import ctypes as C
import numpy as np
from ._lib import lib, _p, Context, LvkError, IMU, PIX_FORMATS, pixfmt_host_array  # noqa: F401


def _u8(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 2
    return img


def _pts(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 2))


def clahe(ctx, img, clip=3.0, tiles=(8, 8)):
    img = _u8(img); h, w = img.shape
    d_src = ctx.to_device(img); d_dst = ctx.alloc(img.nbytes)
    ctx.check(lib().lvk_clahe_u8(ctx.h, _p(d_src), w, h, w, _p(d_dst), w, clip, tiles[0], tiles[1]))
    return ctx.to_host(d_dst, np.uint8, (h, w))


def image_to_gray(ctx, img, fmt, shift=0):
    """lvk_image_to_gray: an image in pixel format `fmt` (the array ImageProcessor.set_input_format describes) -> (H, W) uint8 grey"""
    img = np.ascontiguousarray(pixfmt_host_array(img, fmt))
    h, w = img.shape[:2]
    d_src = ctx.to_device(img); d_dst = ctx.alloc(w * h)
    ctx.check(lib().lvk_image_to_gray(ctx.h, _p(d_src), img.strides[0], w, h, PIX_FORMATS[fmt], int(shift), _p(d_dst), w))
    return ctx.to_host(d_dst, np.uint8, (h, w))


class Pyramid:
    """lvk_pyramid: cv::buildOpticalFlowPyramid(img, win, max_level, withDerivatives=True) on the GPU."""

    def __init__(self, ctx, w, h, win=21, max_level=2):
        self.ctx, self.w, self.h, self.win = ctx, w, h, win
        p = C.c_void_p()
        ctx.check(lib().lvk_pyramid_create(ctx.h, w, h, win, max_level, C.byref(p)))
        self.h_ = p

    def build(self, img, clahe=False, clip=3.0, tiles=(8, 8)):
        img = _u8(img)
        assert img.shape == (self.h, self.w)
        d = self.ctx.to_device(img)
        self.build_device(d, self.w, clahe, clip, tiles)
        self.ctx.sync()
        return self

    def build_device(self, d_img, stride, clahe=False, clip=3.0, tiles=(8, 8)):
        if clahe:
            self.ctx.check(lib().lvk_pyramid_build_clahe(self.ctx.h, self.h_, _p(d_img), stride, clip, tiles[0], tiles[1]))
        else:
            self.ctx.check(lib().lvk_pyramid_build(self.ctx.h, self.h_, _p(d_img), stride))

    @property
    def n_levels(self):
        return lib().lvk_pyramid_levels(self.h_)

    def _level(self, l):
        w, h, pad, ist, dst = (C.c_int() for _ in range(5))
        pi, pd = C.c_void_p(), C.c_void_p()
        st = lib().lvk_pyramid_level(self.h_, l, C.byref(w), C.byref(h), C.byref(pad), C.byref(ist), C.byref(dst), C.byref(pi), C.byref(pd))
        if st != 0:
            raise LvkError("bad level")
        return w.value, h.value, pad.value, ist.value, dst.value, pi.value, pd.value

    def image(self, l, padded=False):
        w, h, pad, ist, _, pi, _ = self._level(l)
        a = self.ctx.to_host(pi, np.uint8, (h + 2 * pad, ist))[:, :w + 2 * pad]
        return a if padded else a[pad:pad + h, pad:pad + w]

    def deriv(self, l, padded=False):
        w, h, pad, _, dst, _, pd = self._level(l)
        a = self.ctx.to_host(pd, np.int16, (h + 2 * pad, dst))[:, :2 * (w + 2 * pad)].reshape(h + 2 * pad, w + 2 * pad, 2)
        return a if padded else a[pad:pad + h, pad:pad + w]

    def orb_prepare(self):
        n = (self.h + 64) * (self.w + 64)
        self.d_ext = self.ctx.alloc(n); self.d_blur = self.ctx.alloc(n)
        self.ctx.check(lib().lvk_orb_prepare(self.ctx.h, self.h_, _p(self.d_ext), _p(self.d_blur)))
        return (self.ctx.to_host(self.d_ext, np.uint8, (self.h + 64, self.w + 64)),
                self.ctx.to_host(self.d_blur, np.uint8, (self.h + 64, self.w + 64)))

    def min_eigen_map(self):
        d = self.ctx.alloc(4 * self.w * self.h)
        self.ctx.check(lib().lvk_min_eigen_map(self.ctx.h, self.h_, _p(d)))
        return self.ctx.to_host(d, np.float32, (self.h, self.w))

    def good_features(self, max_corners, quality=0.01, min_distance=20.0, mask=None):
        cap = max_corners
        d_out = self.ctx.alloc(8 * cap); d_n = self.ctx.alloc(4)
        d_mask = self.ctx.to_device(_u8(mask)) if mask is not None else None
        self.ctx.check(lib().lvk_good_features(self.ctx.h, self.h_, _p(d_mask), max_corners, quality, min_distance, _p(d_out), cap, _p(d_n)))
        n = int(self.ctx.to_host(d_n, np.int32, (1,))[0])
        return self.ctx.to_host(d_out, np.float32, (cap, 2))[:n].copy()

    def close(self):
        if self.h_:
            self.ctx.sync()
            lib().lvk_pyramid_destroy(self.h_)
            self.h_ = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def good_features_from_map(ctx, eig, max_corners, quality=0.01, min_distance=20.0, mask=None, cap=None):
    """lvk_good_features_from_map: corner selection on a float32 response map (H, W); cap (default max_corners) = room in the output list"""
    eig = np.ascontiguousarray(eig, np.float32)
    assert eig.ndim == 2
    h, w = eig.shape
    cap = max_corners if cap is None else cap
    d_eig = ctx.to_device(eig); d_out = ctx.alloc(8 * max(cap, 1)); d_n = ctx.alloc(4)
    d_mask = None
    if mask is not None:
        mask = _u8(mask)
        assert mask.shape == eig.shape
        d_mask = ctx.to_device(mask)
    ctx.check(lib().lvk_good_features_from_map(ctx.h, _p(d_eig), _p(d_mask), w, h, max_corners, quality, min_distance, _p(d_out), cap, _p(d_n)))
    n = int(ctx.to_host(d_n, np.int32, (1,))[0])
    return ctx.to_host(d_out, np.float32, (max(cap, 1), 2))[:n].copy()


def lk_track(ctx, prev, nxt, prev_pts, init_pts, max_iter=30, eps=0.01):
    p0 = _pts(prev_pts); p1 = _pts(init_pts); n = len(p0)
    nl = min(prev.n_levels, nxt.n_levels)
    d0 = ctx.to_device(p0); d1 = ctx.to_device(p1); ds = ctx.alloc(max(n, 1)); di = ctx.alloc(4 * max(n, 1) * nl)
    ctx.check(lib().lvk_lk_track(ctx.h, prev.h_, nxt.h_, _p(d0), _p(d1), _p(ds), n, max_iter, eps, _p(di)))
    return ctx.to_host(d1, np.float32, (n, 2)), ctx.to_host(ds, np.uint8, (n,)), ctx.to_host(di, np.int32, (n, nl))


def orb_describe(ctx, pyr, points):
    """pyr.orb_prepare() must have been called."""
    p = _pts(points); n = len(p)
    dp = ctx.to_device(p); dd = ctx.alloc(32 * max(n, 1)); da = ctx.alloc(4 * max(n, 1))
    ctx.check(lib().lvk_orb_describe(ctx.h, _p(pyr.d_ext), _p(pyr.d_blur), pyr.w, pyr.h, _p(dp), n, _p(dd), _p(da)))
    return ctx.to_host(dd, np.uint8, (n, 32)), ctx.to_host(da, np.float32, (n,))


def hamming_rows(ctx, a, b):
    a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8); n = len(a)
    da = ctx.to_device(a); db = ctx.to_device(b); dd = ctx.alloc(4 * max(n, 1))
    ctx.check(lib().lvk_hamming256_rows(ctx.h, _p(da), _p(db), n, _p(dd)))
    return ctx.to_host(dd, np.int32, (n,))


def orb_match_guided(ctx, cand_pts, cand_desc, q_px, q_radius, q_desc, max_dist=58, ratio_pct=100, check=True):
    """lvk_orb_match_guided: n_q queries (predicted pixel q_px (n_q, 2), search radius q_radius: a number or n_q of them, descriptor q_desc
    (n_q, 32) uint8) against n_cand described corners (cand_pts (n_cand, 2), cand_desc (n_cand, 32)).  -> a MATCH_RESULT array (cand, dist,
    second, n_window, status, pad) whose every byte starts as 0xA5; check=False returns (status code, that array) instead of raising."""
    from ._lib import MATCH_QUERY, MATCH_RESULT
    cp = _pts(cand_pts); cd = np.ascontiguousarray(cand_desc, np.uint8).reshape(-1, 32)
    qp = _pts(q_px); qd = np.ascontiguousarray(q_desc, np.uint8).reshape(-1, 32)
    nc, nq = len(cp), len(qp)
    assert len(cd) == nc and len(qd) == nq
    q = np.zeros(nq, MATCH_QUERY); q["x"] = qp[:, 0]; q["y"] = qp[:, 1]; q["radius"] = q_radius
    res = np.zeros(max(nq, 1), MATCH_RESULT); res.view(np.uint8)[...] = 0xA5
    d_cp = ctx.to_device(cp); d_cd = ctx.to_device(cd); d_q = ctx.to_device(q); d_qd = ctx.to_device(qd); d_res = ctx.to_device(res)
    st = lib().lvk_orb_match_guided(ctx.h, _p(d_cp) if nc else None, _p(d_cd) if nc else None, nc, _p(d_q) if nq else None, _p(d_qd) if nq else None, nq,
                                    int(max_dist), int(ratio_pct), _p(d_res) if nq else None)
    if check:
        ctx.check(st)
    out = ctx.to_host(d_res, MATCH_RESULT, (max(nq, 1),))[:nq].copy() if st == 0 else res[:nq]
    return out if check else (st, out)


ORB_GLOBAL_SLICE, ORB_GLOBAL_TILE = 2048, 256      # GLB_SLICE, GLB_TILE of csrc/fe_global.hip: map points and corners per workgroup of the search
ORB_GLOBAL_GUARD = 64                              # sentinel bytes (0x5A) orb_match_global keeps on either side of every output buffer


def orb_match_global(ctx, map_desc, cand_desc, max_dist=58, ratio_pct=100, max_matches=1024, check=True):
    """lvk_orb_match_global: the frame's described corners cand_desc (n_cand, 32) uint8 against a map's descriptors map_desc (n_map, 32) - a
    host array, or a (DeviceBuffer, n_map) pair for a map that is already on the device.  -> dict(best: n_cand MATCH_RESULT records whose
    cand is the MAP index, sel: the n_selected GLOBAL_MATCH records (cand = corner, index = map point) in (dist, corner) order, info: one
    GLOBAL_INFO record, and best_raw, sel_raw, info_raw: the device buffers as bytes - sel sized for max_matches records - with
    ORB_GLOBAL_GUARD sentinel bytes of 0x5A on either side, every output byte starting as 0x5A too).  check=False returns (status code,
    that dict) instead of raising."""
    from ._lib import MATCH_RESULT, GLOBAL_MATCH, GLOBAL_INFO, DeviceBuffer
    cd = np.ascontiguousarray(cand_desc, np.uint8).reshape(-1, 32); nc = len(cd)
    if isinstance(map_desc, tuple):
        d_map, nm = map_desc
    else:
        md = np.ascontiguousarray(map_desc, np.uint8).reshape(-1, 32); nm = len(md)
        d_map = ctx.to_device(md) if nm else None
    G = ORB_GLOBAL_GUARD
    sizes = dict(best=MATCH_RESULT.itemsize * nc, sel=GLOBAL_MATCH.itemsize * max(min(int(max_matches), 1024), 0), info=GLOBAL_INFO.itemsize)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0x5A, np.uint8)) for k, v in sizes.items()}
    at = lambda k: C.c_void_p(bufs[k].ptr + G)
    d_cd = ctx.to_device(cd) if nc else None
    st = lib().lvk_orb_match_global(ctx.h, _p(d_map), nm, _p(d_cd), nc, int(max_dist), int(ratio_pct), int(max_matches), at("best"), at("sel"), at("info"))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    body = lambda k: raw[k][G:G + sizes[k]]
    info = body("info").view(GLOBAL_INFO)[0]
    ns = int(info["n_selected"]) if st == 0 and nc else 0
    out = dict(best=body("best").view(MATCH_RESULT), sel=body("sel").view(GLOBAL_MATCH)[:ns], info=info, **{k + "_raw": v for k, v in raw.items()})
    return out if check else (st, out)


def align_options(thresh=0.0, min_depth=0.0, min_dz=0.0, min_inliers=0, max_refine_iters=0):
    """lvk_align_options; a zero field takes the library's default (0.01, 0.1, 1e-6, 6, 10)"""
    from ._lib import AlignOptions
    return AlignOptions(float(thresh), float(min_depth), float(min_dz), int(min_inliers), int(max_refine_iters))


def align_draw_pairs(n, max_hypotheses=0, seed=0):
    """lvk_align_draw_pairs (host code): the pairs ImageProcessor.align_landmarks tries for n matches -> an ALIGN_PAIR array"""
    from ._lib import ALIGN_PAIR, ALIGN_MAX_PAIRS
    buf = np.zeros(ALIGN_MAX_PAIRS, ALIGN_PAIR)
    k = lib().lvk_align_draw_pairs(int(n), int(max_hypotheses), int(seed) & 0xFFFFFFFF, _p(buf))
    if k < 0:
        raise ValueError(f"lvk_align_draw_pairs refused n = {n}, max_hypotheses = {max_hypotheses}")
    return buf[:k].copy()


ALIGN_GUARD = 64        # sentinel bytes (0xA5) align_ransac_2pt keeps on either side of the records, the mask and the result


def align_ransac_2pt(ctx, matches, pairs, R_wc, p_wc, options=None, n=None, n_pairs=None, want_hyp=True, check=True):
    """lvk_align_ransac_2pt: matches (an ALIGN_MATCH array: X, u, v) and pairs (ALIGN_PAIR) against the camera pose (R_wc 3 x 3 camera to
    world, p_wc); options: align_options(...) or None.  n / n_pairs default to the arrays' lengths (smaller values leave the tails unread).
    -> dict(hyp: the n_pairs ALIGN_HYP records (None unless want_hyp), mask: n bytes, result: one ALIGN_RESULT record, and hyp_raw,
    mask_raw, result_raw: the device buffers as bytes with ALIGN_GUARD sentinel bytes of 0xA5 on either side, every output byte starting
    as 0xA5 too).  check=False returns (status code, that dict) instead of raising."""
    from ._lib import ALIGN_MATCH, ALIGN_PAIR, ALIGN_HYP, ALIGN_RESULT
    m = np.ascontiguousarray(matches, ALIGN_MATCH); pr = np.ascontiguousarray(pairs, ALIGN_PAIR)
    n = len(m) if n is None else int(n); npr = len(pr) if n_pairs is None else int(n_pairs)
    R = np.ascontiguousarray(R_wc, np.float64).reshape(9); p = np.ascontiguousarray(p_wc, np.float64).reshape(3)
    G = ALIGN_GUARD
    sizes = dict(hyp=ALIGN_HYP.itemsize * max(npr, 0), mask=max(n, 0), result=ALIGN_RESULT.itemsize)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0xA5, np.uint8)) for k, v in sizes.items()}
    d_m = ctx.to_device(m.view(np.uint8) if len(m) else np.zeros(8, np.uint8)); d_pr = ctx.to_device(pr.view(np.uint8) if len(pr) else np.zeros(8, np.uint8))
    st = lib().lvk_align_ransac_2pt(ctx.h, _p(d_m), n, _p(d_pr), npr, _p(R), _p(p), C.byref(options) if options is not None else None,
                                    C.c_void_p(bufs["hyp"].ptr + G) if want_hyp else None, C.c_void_p(bufs["mask"].ptr + G), C.c_void_p(bufs["result"].ptr + G))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    out = dict(hyp=raw["hyp"][G:G + sizes["hyp"]].view(ALIGN_HYP) if want_hyp else None, mask=raw["mask"][G:G + sizes["mask"]],
               result=raw["result"][G:G + sizes["result"]].view(ALIGN_RESULT)[0], hyp_raw=raw["hyp"], mask_raw=raw["mask"], result_raw=raw["result"])
    return out if check else (st, out)


def map_select_options(min_depth=0.0, max_depth=0.0, max_r2=0.0, margin=0.0, k_sigma=0.0, sigma_px=0.0, r_min=0.0, r_max=0.0, rows=0, cols=0, quota=0):
    """lvk_map_select_options; a zero field takes the library's default (0.1, inf, inf, 0, 3, 1, 4, 40, 4 x 5, 1024 / (rows cols))"""
    from ._lib import MapSelectOptions
    return MapSelectOptions(float(min_depth), float(max_depth), float(max_r2), float(margin), float(k_sigma), float(sigma_px), float(r_min), float(r_max),
                            int(rows), int(cols), int(quota), 0)


def map_camera(fe_config):
    """lvk_map_camera of a front-end configuration dict (intrinsics, distortion_model, distortion, width, height)"""
    from ._lib import MapCamera
    return MapCamera((C.c_double * 4)(*fe_config["intrinsics"]), int(fe_config["distortion_model"]), int(fe_config["width"]), int(fe_config["height"]), 0,
                     (C.c_double * 4)(*fe_config["distortion"]))


def align_record(align):
    """an ALIGN_RESULT record for an alignment given as one (returned as it is), as (c, s, t) or as None (-> None: identity)"""
    from ._lib import ALIGN_RESULT
    if align is None or (isinstance(align, (np.ndarray, np.void)) and align.dtype == ALIGN_RESULT):
        return None if align is None else np.ascontiguousarray(align, ALIGN_RESULT).reshape(1)
    r = np.zeros(1, ALIGN_RESULT)
    r["c"], r["s"], r["t"] = float(align[0]), float(align[1]), np.asarray(align[2], np.float64).reshape(3)
    return r


MAP_GUARD = 64          # sentinel bytes (0xA5) map_select_queries keeps on either side of every output buffer


def map_select_queries(ctx, X, cov, desc, fe_config, R_wc, p_wc, align=None, cov_cam=None, options=None, want_status=True, check=True):
    """lvk_map_select_queries over host arrays: X (n, 3) map points, cov (n, 3, 3) or None, desc (n, 32) uint8 or None, the camera of
    fe_config, the pose (R_wc 3 x 3 camera to world, p_wc), align: None, an ALIGN_RESULT record or (c, s, t), cov_cam: None or 6 x 6,
    options: map_select_options(...) or None.  -> dict(info: one MAP_INFO record, sel: the n_selected MAP_SEL records, q: the MATCH_QUERY
    records, q_desc: (n_selected, 32) uint8 or None, status: (n,) uint8 or None, and sel_raw, q_raw, q_desc_raw, info_raw, status_raw: the
    device buffers as bytes, sized for 1024 records, with MAP_GUARD sentinel bytes of 0xA5 on either side, every output byte starting as
    0xA5 too).  check=False returns (status code, that dict) instead of raising."""
    from ._lib import MAP_SEL, MAP_INFO, MATCH_QUERY, MAP_MAX_QUERIES
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); n = len(X)
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
    ds = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    assert (cv is None or len(cv) == n) and (ds is None or len(ds) == n)
    R = np.ascontiguousarray(R_wc, np.float64).reshape(9); p = np.ascontiguousarray(p_wc, np.float64).reshape(3)
    cc = None if cov_cam is None else np.ascontiguousarray(cov_cam, np.float64).reshape(36)
    al = align_record(align); cam = map_camera(fe_config)
    G = MAP_GUARD
    sizes = dict(sel=MAP_SEL.itemsize * MAP_MAX_QUERIES, q=MATCH_QUERY.itemsize * MAP_MAX_QUERIES, q_desc=32 * MAP_MAX_QUERIES, info=MAP_INFO.itemsize, status=n)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0xA5, np.uint8)) for k, v in sizes.items()}
    at = lambda k: C.c_void_p(bufs[k].ptr + G)
    d_X = ctx.to_device(X) if n else None; d_cov = ctx.to_device(cv) if cv is not None and n else None; d_desc = ctx.to_device(ds) if ds is not None and n else None
    st = lib().lvk_map_select_queries(ctx.h, _p(d_X), _p(d_cov), _p(d_desc), n, C.byref(cam), _p(al), _p(R), _p(p), _p(cc), C.byref(options) if options is not None else None,
                                      at("sel"), at("q"), at("q_desc") if ds is not None else None, at("info"), at("status") if want_status else None)
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    body = lambda k: raw[k][G:G + sizes[k]]
    info = body("info").view(MAP_INFO)[0]
    ns = int(info["n_selected"]) if st == 0 else 0
    out = dict(info=info, sel=body("sel").view(MAP_SEL)[:ns], q=body("q").view(MATCH_QUERY)[:ns], q_desc=body("q_desc").reshape(-1, 32)[:ns] if ds is not None else None,
               status=body("status") if want_status else None, **{k + "_raw": v for k, v in raw.items()})
    return out if check else (st, out)


def map_build_options(max_score=0.0, r_dup=0.0, dup_max_dist=0):
    """lvk_map_build_options; a zero field takes the library's default (inf, 0 = no de-duplication, 32)"""
    from ._lib import MapBuildOptions
    return MapBuildOptions(float(max_score), float(r_dup), int(dup_max_dist), 0)


MAP_BUILD_GUARD = 64    # sentinel bytes (0xA5) map_build keeps on either side of every output buffer


def map_build(ctx, X, cov, desc, score=None, options=None, want_status=True, check=True):
    """lvk_map_build over host arrays: X (n, 3) raw map points, cov (n, 3, 3) or None, desc (n, 32) uint8 or None, score (n,) or None
    (smaller is better), options: map_build_options(...) or None.  -> dict(info: one MAP_BUILD_INFO record, order: the n_kept original
    indices best first, X, cov, desc: the kept points gathered in that order (cov / desc None when not given), status: (n,) uint8 or None,
    and order_raw, X_raw, cov_raw, desc_raw, status_raw, info_raw: the device buffers as bytes, sized for n records, with MAP_BUILD_GUARD
    sentinel bytes of 0xA5 on either side, every output byte starting as 0xA5 too).  check=False returns (status code, that dict) instead
    of raising."""
    from ._lib import MAP_BUILD_INFO
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); n = len(X)
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
    ds = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    sc = None if score is None else np.ascontiguousarray(score, np.float64).reshape(-1)
    assert (cv is None or len(cv) == n) and (ds is None or len(ds) == n) and (sc is None or len(sc) == n)
    G = MAP_BUILD_GUARD
    sizes = dict(order=4 * n, X=24 * n, cov=72 * n if cv is not None else 0, desc=32 * n if ds is not None else 0, status=n, info=MAP_BUILD_INFO.itemsize)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0xA5, np.uint8)) for k, v in sizes.items()}
    at = lambda k: C.c_void_p(bufs[k].ptr + G)
    dev = [ctx.to_device(a) if a is not None and n else None for a in (X, cv, ds, sc)]
    st = lib().lvk_map_build(ctx.h, _p(dev[0]), _p(dev[1]), _p(dev[2]), _p(dev[3]), n, C.byref(options) if options is not None else None, at("order"), at("X"),
                             at("cov") if cv is not None else None, at("desc") if ds is not None else None, at("status") if want_status else None, at("info"))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    body = lambda k: raw[k][G:G + sizes[k]]
    info = body("info").view(MAP_BUILD_INFO)[0]
    nk = int(info["n_kept"]) if st == 0 else 0
    out = dict(info=info, order=body("order").view(np.int32)[:nk], X=body("X").view(np.float64).reshape(-1, 3)[:nk],
               cov=body("cov").view(np.float64).reshape(-1, 3, 3)[:nk] if cv is not None else None, desc=body("desc").reshape(-1, 32)[:nk] if ds is not None else None,
               status=body("status") if want_status else None, **{k + "_raw": v for k, v in raw.items()})
    return out if check else (st, out)


def align3d_options(thresh=0.0, min_rho=0.0, min_inliers=0):
    """lvk_align3d_options; a zero field takes the library's default (0.10 m, 0.5 m, 6)"""
    from ._lib import Align3dOptions
    return Align3dOptions(float(thresh), float(min_rho), int(min_inliers), 0)


def align_invert(align):
    """lvk_align_invert (host code): the alignment the other way round.  align: an ALIGN_RESULT record or (c, s, t) -> one ALIGN_RESULT record"""
    from ._lib import ALIGN_RESULT
    a = align_record(align)
    if a is None:
        raise ValueError("align_invert needs an alignment")
    out = np.zeros(1, ALIGN_RESULT)
    if lib().lvk_align_invert(_p(a), _p(out)) != 0:
        raise ValueError("lvk_align_invert refused its arguments")
    return out[0]


def align_ransac_3d(ctx, matches, pairs, options=None, n=None, n_pairs=None, want_hyp=True, check=True):
    """lvk_align_ransac_3d: matches (an ALIGN3D_MATCH array: X in session B's frame, Y in the map's) and pairs (ALIGN_PAIR); options:
    align3d_options(...) or None.  n / n_pairs default to the arrays' lengths (smaller values leave the tails unread).
    -> dict(hyp: the n_pairs ALIGN3D_HYP records (None unless want_hyp), mask: n bytes, result: one ALIGN_RESULT record, and hyp_raw,
    mask_raw, result_raw: the device buffers as bytes with ALIGN_GUARD sentinel bytes of 0xA5 on either side, every output byte starting
    as 0xA5 too).  check=False returns (status code, that dict) instead of raising."""
    from ._lib import ALIGN3D_MATCH, ALIGN_PAIR, ALIGN3D_HYP, ALIGN_RESULT
    m = np.ascontiguousarray(matches, ALIGN3D_MATCH); pr = np.ascontiguousarray(pairs, ALIGN_PAIR)
    n = len(m) if n is None else int(n); npr = len(pr) if n_pairs is None else int(n_pairs)
    G = ALIGN_GUARD
    sizes = dict(hyp=ALIGN3D_HYP.itemsize * max(npr, 0), mask=max(n, 0), result=ALIGN_RESULT.itemsize)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0xA5, np.uint8)) for k, v in sizes.items()}
    d_m = ctx.to_device(m.view(np.uint8) if len(m) else np.zeros(8, np.uint8)); d_pr = ctx.to_device(pr.view(np.uint8) if len(pr) else np.zeros(8, np.uint8))
    st = lib().lvk_align_ransac_3d(ctx.h, _p(d_m), n, _p(d_pr), npr, C.byref(options) if options is not None else None,
                                   C.c_void_p(bufs["hyp"].ptr + G) if want_hyp else None, C.c_void_p(bufs["mask"].ptr + G), C.c_void_p(bufs["result"].ptr + G))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    out = dict(hyp=raw["hyp"][G:G + sizes["hyp"]].view(ALIGN3D_HYP) if want_hyp else None, mask=raw["mask"][G:G + sizes["mask"]],
               result=raw["result"][G:G + sizes["result"]].view(ALIGN_RESULT)[0], hyp_raw=raw["hyp"], mask_raw=raw["mask"], result_raw=raw["result"])
    return out if check else (st, out)


MAP_TRANSFORM_GUARD = 64    # sentinel bytes (0xA5) map_transform keeps behind every output buffer


def map_transform(ctx, X, cov=None, desc=None, align=None, cov_align=None, head=0, check=True):
    """lvk_map_transform over host arrays: X (n, 3), cov (n, 3, 3) or None, desc (n, 32) uint8 or None, align: None, an ALIGN_RESULT record
    or (c, s, t), cov_align: None or the 4 x 4 covariance of (psi, t).  The outputs are written as the tails of larger buffers: `head`
    records of 0xA5 in front, MAP_TRANSFORM_GUARD bytes of 0xA5 behind.  -> dict(X (n, 3), cov (n, 3, 3) or None, desc (n, 32) or None, and
    X_raw, cov_raw, desc_raw: the whole buffers as bytes).  check=False returns (status code, that dict) instead of raising."""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); n = len(X)
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
    ds = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    assert (cv is None or len(cv) == n) and (ds is None or len(ds) == n)
    P = None if cov_align is None else np.ascontiguousarray(cov_align, np.float64).reshape(16)
    al = align_record(align)
    G, h = MAP_TRANSFORM_GUARD, int(head)
    rec = dict(X=24, cov=72, desc=32)
    have = dict(X=True, cov=cv is not None or P is not None, desc=ds is not None)
    bufs = {k: ctx.to_device(np.full(rec[k] * (h + n) + G, 0xA5, np.uint8)) for k in rec}
    at = lambda k: C.c_void_p(bufs[k].ptr + rec[k] * h) if have[k] else None
    dev = [ctx.to_device(a) if a is not None and n else None for a in (X, cv, ds)]
    st = lib().lvk_map_transform(ctx.h, _p(dev[0]), _p(dev[1]), _p(dev[2]), n, _p(al), _p(P), at("X"), at("cov"), at("desc"))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (rec[k] * (h + n) + G,)).copy() for k in rec}
    body = lambda k: raw[k][rec[k] * h:rec[k] * (h + n)]
    out = dict(X=body("X").view(np.float64).reshape(-1, 3), cov=body("cov").view(np.float64).reshape(-1, 3, 3) if have["cov"] else None,
               desc=body("desc").reshape(-1, 32) if have["desc"] else None, **{k + "_raw": v for k, v in raw.items()})
    return out if check else (st, out)


def undistort(ctx, points, intr, model, dist, new_intr):
    p = _pts(points); n = len(p)
    a = np.asarray(intr, np.float64); d = np.asarray(dist, np.float64); k = np.asarray(new_intr, np.float64)
    dp = ctx.to_device(p); do = ctx.alloc(8 * max(n, 1))
    ctx.check(lib().lvk_undistort_points(ctx.h, _p(dp), n, _p(a), model, _p(d), _p(k), _p(do)))
    return ctx.to_host(do, np.float32, (n, 2))


def find_fundamental_mask(ctx, p1, p2, thresh=1.0, conf=0.99):
    a = _pts(p1); b = _pts(p2); n = len(a)
    da = ctx.to_device(a); db = ctx.to_device(b); dm = ctx.alloc(max(n, 1)); di = ctx.alloc(8)
    ctx.check(lib().lvk_find_fundamental_mask(ctx.h, _p(da), _p(db), n, thresh, conf, _p(dm), _p(di)))
    info = ctx.to_host(di, np.int32, (2,))
    return (ctx.to_host(dm, np.uint8, (n,)) if info[0] else None), int(info[1])


def find_fundamental(ctx, p1, p2, thresh=1.0, conf=0.99):
    """lvk_find_fundamental: -> (mask or None, F 3x3, hypotheses drawn); F = the matrix cv::findFundamentalMat returns (zeros: the empty Mat)"""
    a = _pts(p1); b = _pts(p2); n = len(a)
    da = ctx.to_device(a); db = ctx.to_device(b); dm = ctx.alloc(max(n, 1)); di = ctx.alloc(8); dF = ctx.alloc(72)
    ctx.check(lib().lvk_find_fundamental(ctx.h, _p(da), _p(db), n, thresh, conf, _p(dm), _p(di), _p(dF)))
    info = ctx.to_host(di, np.int32, (2,))
    return (ctx.to_host(dm, np.uint8, (n,)) if info[0] else None), ctx.to_host(dF, np.float64, (3, 3)), int(info[1])


def ransac_fundamental(ctx, p1, p2, thresh=1.0, conf=0.99, max_iters=1000):
    a = _pts(p1); b = _pts(p2); n = len(a)
    da = ctx.to_device(a); db = ctx.to_device(b); dm = ctx.alloc(max(n, 1)); di = ctx.alloc(8)
    ctx.check(lib().lvk_ransac_fundamental(ctx.h, _p(da), _p(db), n, thresh, conf, max_iters, _p(dm), _p(di)))
    info = ctx.to_host(di, np.int32, (2,))
    return ctx.to_host(dm, np.uint8, (n,)), int(info[1])


def predict_homography(imu, t_prev, t_curr, R_cam_imu, intr):
    imu = np.ascontiguousarray(imu, IMU)
    R = np.ascontiguousarray(R_cam_imu, np.float64); k = np.asarray(intr, np.float64)
    H = np.empty(9, np.float32)
    st = lib().lvk_predict_homography(_p(imu), len(imu), t_prev, t_curr, _p(R), _p(k), _p(H))
    if st != 0:
        raise LvkError("lvk_predict_homography")
    return H.reshape(3, 3)


LANDMARK_JOB = np.dtype([("anchor_col", np.int32), ("feat_col", np.int32), ("pad0", np.int32), ("pad1", np.int32), ("q_anchor", np.float64, 4),
                         ("R_b2c", np.float64, 9), ("t_c_b", np.float64, 3), ("obs_anchor", np.float64, 2), ("inv_depth", np.float64)])


def landmark_cov(ctx, P, jobs, n=None):
    """lvk_ekf_landmark_cov: the 3 x 3 position covariance of every LANDMARK_JOB record, read off the covariance P.  P: a whole
    row-major buffer (its row length is the leading dimension, contents go to the device as they are) whose leading n x n block
    (default: all rows) is the covariance.  -> (n_jobs, 3, 3)"""
    P = np.ascontiguousarray(P, np.float64); jobs = np.ascontiguousarray(jobs, LANDMARK_JOB)
    n = P.shape[0] if n is None else int(n)
    out = np.full((len(jobs), 3, 3), np.nan)
    L = lib()
    L.lvk_ekf_landmark_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]; L.lvk_ekf_landmark_cov.restype = C.c_int
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_landmark_cov(ctx.h, _p(dP), P.shape[1], n, _p(jobs), len(jobs), _p(out)))
    return out


POSE_REL_JOB = np.dtype([("a_theta_col", np.int32), ("a_p_col", np.int32), ("b_theta_col", np.int32), ("b_p_col", np.int32), ("q_a", np.float64, 4),
                         ("p_a", np.float64, 3), ("q_b", np.float64, 4), ("p_b", np.float64, 3)])


def pose_rel_cov(ctx, P, jobs, n=None):
    """lvk_ekf_pose_rel_cov: the 6 x 6 covariance of every POSE_REL_JOB record - pose b relative to pose a, or b's own block when
    a_theta_col < 0 - read off the covariance P.  P: a whole row-major buffer (its row length is the leading dimension, contents go to
    the device as they are) whose leading n x n block (default: all rows) is the covariance.  -> (n_jobs, 6, 6)"""
    P = np.ascontiguousarray(P, np.float64); jobs = np.ascontiguousarray(jobs, POSE_REL_JOB)
    n = P.shape[0] if n is None else int(n)
    out = np.full((len(jobs), 6, 6), np.nan)
    L = lib()
    L.lvk_ekf_pose_rel_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]; L.lvk_ekf_pose_rel_cov.restype = C.c_int
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_pose_rel_cov(ctx.h, _p(dP), P.shape[1], n, _p(jobs), len(jobs), _p(out)))
    return out


LANDMARK_REL_JOB = np.dtype(LANDMARK_JOB.descr + [("b_theta_col", np.int32), ("b_p_col", np.int32), ("q_b", np.float64, 4), ("p_b", np.float64, 3),
                                                 ("p_anchor", np.float64, 3)])


def landmark_rel_cov(ctx, P, jobs, n=None):
    """lvk_ekf_landmark_rel_cov: every LANDMARK_REL_JOB record's point in the camera frame of the job's target pose and its 3 x 3
    covariance there, read off the covariance P.  P: a whole row-major buffer (its row length is the leading dimension, contents go to
    the device as they are) whose leading n x n block (default: all rows) is the covariance.  -> (p_c (n_jobs, 3), Sigma (n_jobs, 3, 3))"""
    P = np.ascontiguousarray(P, np.float64); jobs = np.ascontiguousarray(jobs, LANDMARK_REL_JOB)
    n = P.shape[0] if n is None else int(n)
    out = np.full((len(jobs), 12), np.nan)
    L = lib()
    L.lvk_ekf_landmark_rel_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]; L.lvk_ekf_landmark_rel_cov.restype = C.c_int
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_landmark_rel_cov(ctx.h, _p(dP), P.shape[1], n, _p(jobs), len(jobs), _p(out)))
    return np.ascontiguousarray(out[:, :3]), np.ascontiguousarray(out[:, 3:]).reshape(-1, 3, 3)


MSCKF_POINT_JOB = np.dtype([("n_obs", np.int32), ("obs_off", np.int32), ("p_w", np.float64, 3)])


def msckf_point_cov(ctx, P, clones, jobs, clone_rank, obs, obs_vel, leg_dim=22, if_fej=False, estimate_td=False, sigma2=1.0, n=None):
    """lvk_ekf_msckf_point_cov: the 3 x 3 position covariance of every MSCKF_POINT_JOB record (a least-squares point with its
    observations at obs_off + k of clone_rank / obs / obs_vel), read off the covariance P.  P: a whole row-major buffer (its row
    length is the leading dimension, contents go to the device as they are) whose leading n x n block (default: all rows) is the
    covariance; clones: an array of larvio.CLONE records.  -> (Sigma (n_jobs, 3, 3), ok (n_jobs,))"""
    from .larvio import CLONE
    P = np.ascontiguousarray(P, np.float64); jobs = np.ascontiguousarray(jobs, MSCKF_POINT_JOB); clones = np.ascontiguousarray(clones, CLONE)
    rk = np.ascontiguousarray(clone_rank, np.int32); z = np.ascontiguousarray(obs, np.float64); zv = np.ascontiguousarray(obs_vel, np.float64)
    n = P.shape[0] if n is None else int(n)
    out = np.full((len(jobs), 3, 3), np.nan); ok = np.full(len(jobs), -1, np.int32)
    L = lib()
    vp, i = C.c_void_p, C.c_int
    L.lvk_ekf_msckf_point_cov.argtypes = [vp, vp, i, i, vp, i, vp, i, vp, vp, vp, i, i, i, C.c_double, vp, vp]; L.lvk_ekf_msckf_point_cov.restype = i
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_msckf_point_cov(ctx.h, _p(dP), P.shape[1], n, _p(clones), len(clones), _p(jobs), len(jobs), _p(rk), _p(z), _p(zv),
                                        int(leg_dim), int(bool(if_fej)), int(bool(estimate_td)), float(sigma2), _p(out), _p(ok)))
    return out, ok


# lvk_sparse_update (include/lvk_c.h): H is m x ncols packed row-major at the front of its 72 doubles, R m x m packed at the front of its 36
SPARSE_UPDATE = np.dtype([("m", np.int32), ("ncols", np.int32), ("cols", np.int32, 12), ("H", np.float64, 72), ("r", np.float64, 6), ("R", np.float64, 36),
                          ("gate", np.float64)])


def sparse_update_record(cols, H, r, R, gate=0.0, fill=0.0):
    """one SPARSE_UPDATE record from H (m x ncols), r (m), R (m x m); fill: what the entries the call never reads hold"""
    H = np.asarray(H, np.float64); r = np.asarray(r, np.float64); R = np.asarray(R, np.float64)
    m, nc = H.shape
    u = np.zeros(1, SPARSE_UPDATE)
    u["cols"] = -1 if np.isnan(fill) else 0
    u["H"] = fill; u["r"] = fill; u["R"] = fill
    u["m"] = m; u["ncols"] = nc; u["cols"][0, :nc] = cols
    u["H"][0, :m * nc] = H.ravel(); u["r"][0, :m] = r; u["R"][0, :m * m] = R.ravel(); u["gate"] = gate
    return u


def update_sparse(ctx, P, u, n=None):
    """lvk_ekf_update_sparse: one SPARSE_UPDATE record applied to the covariance P.  P: a whole row-major buffer (its row length is
    the leading dimension, contents go to the device as they are) whose leading n x n block (default: all rows) is the covariance.
    -> (dx (n,), the whole P buffer after the call, info (4,): status, gamma, smallest pivot, 0)"""
    P = np.ascontiguousarray(P, np.float64); u = np.ascontiguousarray(u, SPARSE_UPDATE)
    n = P.shape[0] if n is None else int(n)
    dx = np.full(n, np.nan); info = np.full(4, np.nan)
    L = lib()
    L.lvk_ekf_update_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]; L.lvk_ekf_update_sparse.restype = C.c_int
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_update_sparse(ctx.h, _p(dP), P.shape[1], n, _p(u), _p(dx), _p(info)))
    return dx, ctx.to_host(dP, np.float64, P.shape), info


# ---- stage entries of the frame path (include/lvk_c.h: lvk_fe_track_stage, lvk_fe_commit_stage, lvk_fe_msg_stage)
class FeTrackIo(C.Structure):
    _fields_ = [("n", C.c_int), ("grid", C.c_int), ("is_new", C.c_int), ("h_src_pts", C.c_void_p), ("h_stored_desc", C.c_void_p),
                ("h_curr", C.c_void_p), ("h_status", C.c_void_p), ("h_und", C.c_void_p), ("h_desc", C.c_void_p)]


class FeTrackArrays(C.Structure):
    _fields_ = [("id", C.c_void_p), ("pts", C.c_void_p), ("ppts", C.c_void_p), ("init", C.c_void_p), ("life", C.c_void_p), ("desc", C.c_void_p)]


class FeCommitState(C.Structure):
    _fields_ = [("next_id", C.c_uint64), ("dst_n", C.c_int), ("n_new", C.c_int), ("boot_ok", C.c_int)]


class FeMsgState(C.Structure):
    _fields_ = [("n_msg", C.c_int), ("n_host", C.c_int), ("msg_features", C.c_uint64), ("msg_count", C.c_uint64)]


def _hp(a):
    return a.ctypes.data if a is not None else None


def _finish(ctx, st, check):
    if check:
        ctx.check(st)
    return st


def fe_track_stage(ctx, prev, nxt, sets, patch_size, variant, H, model, intr, dist, max_iteration=30, track_precision=0.01,
                   fill=0xA5, counters=(0, 0), width=None, height=None, check=True):
    """lvk_fe_track_stage.  prev / nxt: built Pyramids whose orb_prepare() has run.  sets: one or two dicts with pts (n, 2), grid (slots,
    default n), is_new and - for old tracks - stored_desc (n, 32) uint8; a key `n` overrides the count.  -> (status, [dict(curr (grid, 2), status (grid,),
    und (grid, 2, 2), desc (grid, 32) or None)], (point_levels, iterations)); every output array starts as the byte `fill`."""
    L = lib()
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    L.lvk_fe_track_stage.argtypes = [vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp, i, vp, vp, i, d, i, vp, vp, vp]; L.lvk_fe_track_stage.restype = i
    ios, outs, keep = [], [], []
    for s in sets:
        p = _pts(s["pts"]); n = int(s.get("n", len(p))); grid = int(s.get("grid", len(p))); is_new = int(s["is_new"])
        sd = None if s.get("stored_desc") is None else np.ascontiguousarray(s["stored_desc"], np.uint8)
        g = max(grid, 1)
        o = dict(curr=np.full((g, 2), 0, np.float32), status=np.full(g, fill, np.uint8), und=np.zeros((g, 2, 2), np.float32),
                 desc=np.full((g, 32), fill, np.uint8) if is_new == 1 else None)
        o["curr"].view(np.uint8)[...] = fill; o["und"].view(np.uint8)[...] = fill
        if s.get("null_out"):
            o["curr"] = None
        ios.append(FeTrackIo(n, grid, is_new, _hp(p), _hp(sd), _hp(o["curr"]), _hp(o["status"]), _hp(o["und"]), _hp(o["desc"])))
        keep += [p, sd]; outs.append(o)
    Hc = None if H is None else np.ascontiguousarray(H, np.float32).reshape(9)
    a = np.asarray(intr, np.float64); dd = np.asarray(dist, np.float64)
    cnt = np.array(counters, np.uint64)
    st = L.lvk_fe_track_stage(ctx.h, prev.h_, nxt.h_, _p(prev.d_ext), _p(prev.d_blur), _p(nxt.d_ext), _p(nxt.d_blur),
                              prev.w if width is None else width, prev.h if height is None else height, patch_size, variant, _p(Hc), model, _p(a), _p(dd),
                              max_iteration, track_precision, fill, C.byref(ios[0]), C.byref(ios[1]) if len(ios) > 1 else None, _p(cnt))
    _finish(ctx, st, check)
    for o, s in zip(outs, ios):
        for k in ("curr", "status", "und", "desc"):
            if o[k] is not None:
                o[k] = o[k][:s.grid]
    return st, outs, (int(cnt[0]), int(cnt[1]))


def track_set_arrays(cap, fill=0xA5):
    """a track set of cap slots whose every byte is `fill`: dict(id, pts, ppts, init, life, desc)"""
    t = dict(id=np.zeros(cap, np.uint64), pts=np.zeros((cap, 2), np.float32), ppts=np.zeros((cap, 2), np.float32), init=np.zeros((cap, 2), np.float32),
             life=np.zeros(cap, np.int32), desc=np.zeros((cap, 32), np.uint8))
    for v in t.values():
        v.view(np.uint8)[...] = fill
    return t


def _track_arrays(t):
    return FeTrackArrays(*[_hp(t.get(k)) for k in ("id", "pts", "ppts", "init", "life", "desc")])


def fe_commit_stage(ctx, mode, cap, src, dst, state, n=None, check=True):
    """lvk_fe_commit_stage.  src: dict(pts (n, 2), curr (n, 2), status (n,), und (n, 2, 2), desc (n, 32) and, mode 0, id, init, life); dst: a
    track_set_arrays(cap) dict, updated in place; state: dict(next_id, dst_n, n_new, boot_ok), a new one is returned.  -> (status, state)"""
    L = lib()
    vp, i = C.c_void_p, C.c_int
    L.lvk_fe_commit_stage.argtypes = [vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]; L.lvk_fe_commit_stage.restype = i
    f32 = lambda k, shape: None if src.get(k) is None else np.ascontiguousarray(src[k], np.float32).reshape(shape)
    p, c, u, ini = f32("pts", (-1, 2)), f32("curr", (-1, 2)), f32("und", (-1, 2, 2)), f32("init", (-1, 2))
    stt = None if src.get("status") is None else np.ascontiguousarray(src["status"], np.uint8)
    ids = None if src.get("id") is None else np.ascontiguousarray(src["id"], np.uint64)
    life = None if src.get("life") is None else np.ascontiguousarray(src["life"], np.int32)
    desc = None if src.get("desc") is None else np.ascontiguousarray(src["desc"], np.uint8)
    n = len(stt) if n is None else int(n)
    cs = FeCommitState(int(state["next_id"]), int(state["dst_n"]), int(state["n_new"]), int(state["boot_ok"]))
    ta = _track_arrays(dst)
    st = L.lvk_fe_commit_stage(ctx.h, mode, cap, n, _hp(p), _hp(c), _hp(stt), _hp(u), _hp(ids), _hp(ini), _hp(life), _hp(desc), C.byref(ta), C.byref(cs))
    _finish(ctx, st, check)
    return st, dict(next_id=int(cs.next_id), dst_n=cs.dst_n, n_new=cs.n_new, boot_ok=cs.boot_ok)


def fe_msg_stage(ctx, tset, cap, n, model, intr, dist, dt_1, dt_2, prev_is_last, state, fill=0xA5, check=True):
    """lvk_fe_msg_stage.  tset: dict(id, pts, ppts, init) of cap slots, init updated in place; state: dict(n_msg, n_host, msg_features,
    msg_count), a new one is returned.  -> (status, message (cap,) OBS records whose slots >= n keep the byte `fill`, state)"""
    from ._lib import OBS
    L = lib()
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    L.lvk_fe_msg_stage.argtypes = [vp, vp, i, i, i, vp, vp, d, d, i, i, vp, vp]; L.lvk_fe_msg_stage.restype = i
    out = np.zeros(max(cap, 1), OBS); out.view(np.uint8)[...] = fill
    ms = FeMsgState(int(state["n_msg"]), int(state["n_host"]), int(state["msg_features"]), int(state["msg_count"]))
    ta = _track_arrays(tset)
    a = np.asarray(intr, np.float64); dd = np.asarray(dist, np.float64)
    st = L.lvk_fe_msg_stage(ctx.h, C.byref(ta), cap, n, model, _p(a), _p(dd), dt_1, dt_2, prev_is_last, fill, _p(out), C.byref(ms))
    _finish(ctx, st, check)
    return st, out[:max(cap, 0)], dict(n_msg=ms.n_msg, n_host=ms.n_host, msg_features=int(ms.msg_features), msg_count=int(ms.msg_count))


# lvk_landmark_fix_job / lvk_landmark_obs (include/lvk_c.h)
LANDMARK_FIX_JOB = np.dtype([("clone_col", np.int32), ("pad0", np.int32), ("q_b", np.float64, 4), ("p_b", np.float64, 3), ("R_b2c", np.float64, 9), ("t_c_b", np.float64, 3),
                             ("gate", np.float64), ("min_depth", np.float64)])
LANDMARK_OBS = np.dtype([("p_w", np.float64, 3), ("cov_w", np.float64, 9), ("uv", np.float64, 2), ("sigma", np.float64)])


def update_landmarks(ctx, P, job, obs, n=None):
    """lvk_ekf_update_landmarks: one LANDMARK_FIX_JOB record and a LANDMARK_OBS array applied to the covariance P.  P: a whole row-major
    buffer (its row length is the leading dimension, contents go to the device as they are) whose leading n x n block (default: all
    rows) is the covariance.  -> (dx (n,), the whole P buffer after the call, info (8,), status (n_obs,), gamma (n_obs,))"""
    P = np.ascontiguousarray(P, np.float64); job = np.ascontiguousarray(job, LANDMARK_FIX_JOB); obs = np.ascontiguousarray(obs, LANDMARK_OBS)
    n = P.shape[0] if n is None else int(n)
    dx = np.full(n, np.nan); info = np.full(8, np.nan); st = np.full(max(len(obs), 1), -1, np.int32); g = np.full(max(len(obs), 1), np.nan)
    L = lib()
    vp, i = C.c_void_p, C.c_int
    L.lvk_ekf_update_landmarks.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, vp, vp]; L.lvk_ekf_update_landmarks.restype = i
    dP = ctx.to_device(P)
    ctx.check(L.lvk_ekf_update_landmarks(ctx.h, _p(dP), P.shape[1], n, _p(job), _p(obs) if len(obs) else None, len(obs), _p(dx), _p(info), _p(st), _p(g)))
    return dx, ctx.to_host(dP, np.float64, P.shape), info, st[:len(obs)], g[:len(obs)]


# lvk_camera_pose_job (include/lvk_c.h): LANDMARK_FIX_JOB without the gate fields
CAMERA_POSE_JOB = np.dtype([("clone_col", np.int32), ("pad0", np.int32), ("q_b", np.float64, 4), ("p_b", np.float64, 3), ("R_b2c", np.float64, 9), ("t_c_b", np.float64, 3)])


def camera_pose_job(clone_col, q_b, p_b, R_b2c, t_c_b):
    """one CAMERA_POSE_JOB record"""
    j = np.zeros(1, CAMERA_POSE_JOB)
    j["clone_col"] = int(clone_col); j["q_b"] = np.asarray(q_b, np.float64).reshape(4); j["p_b"] = np.asarray(p_b, np.float64).reshape(3)
    j["R_b2c"] = np.asarray(R_b2c, np.float64).reshape(9); j["t_c_b"] = np.asarray(t_c_b, np.float64).reshape(3)
    return j


def camera_pose_cov(ctx, P, job, n=None, check=True):
    """lvk_ekf_camera_pose_cov: the camera pose of the CAMERA_POSE_JOB record's clone and its 6 x 6 covariance [dtheta dp], read off the
    covariance P.  P: a whole row-major buffer (its row length is the leading dimension, contents go to the device as they are) whose
    leading n x n block (default: all rows) is the covariance.  -> (R_wc (3, 3), p_wc (3,), cov_cam (6, 6)); check=False returns
    (status code, that triple) instead of raising - the outputs keep their NaN fill when the call is refused."""
    P = np.ascontiguousarray(P, np.float64); job = np.ascontiguousarray(job, CAMERA_POSE_JOB).reshape(1)
    n = P.shape[0] if n is None else int(n)
    R = np.full((3, 3), np.nan); p = np.full(3, np.nan); cov = np.full((6, 6), np.nan)
    dP = ctx.to_device(P)
    st = lib().lvk_ekf_camera_pose_cov(ctx.h, _p(dP), P.shape[1], n, _p(job), _p(R), _p(p), _p(cov))
    if check:
        ctx.check(st)
        return R, p, cov
    return st, (R, p, cov)


MAP_OBS_GUARD = 64      # sentinel bytes (0xA5) map_gather_obs keeps on either side of every output buffer


def map_gather_obs(ctx, records, X, cov, sigma, align=None, n_rec=None, check=True):
    """lvk_map_gather_obs over host arrays: records (a MAP_MATCH array, as match_map returns it), the map X (n_map, 3) with cov
    (n_map, 3, 3) or None, sigma in normalised units, align: None, an ALIGN_RESULT record or (c, s, t).  -> dict(info: one MAP_OBS_INFO
    record, obs: the n_ok LANDMARK_OBS rows, idx: the rows of `records` they came from, and obs_raw, idx_raw, info_raw: the device buffers
    as bytes, sized for n_rec entries, with MAP_OBS_GUARD sentinel bytes of 0xA5 on either side, every output byte starting as 0xA5 too).
    n_rec: the count handed to the library when it is not len(records).  check=False returns (status code, that dict) instead of raising."""
    from ._lib import MAP_MATCH, MAP_OBS_INFO
    rec = np.ascontiguousarray(records, MAP_MATCH).reshape(-1)
    nr = len(rec) if n_rec is None else int(n_rec)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); n_map = len(X)
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(-1, 9)
    assert cv is None or len(cv) == n_map
    al = align_record(align)
    G = MAP_OBS_GUARD; room = max(len(rec), 1)
    sizes = dict(obs=LANDMARK_OBS.itemsize * room, idx=4 * room, info=MAP_OBS_INFO.itemsize)
    bufs = {k: ctx.to_device(np.full(v + 2 * G, 0xA5, np.uint8)) for k, v in sizes.items()}
    at = lambda k: C.c_void_p(bufs[k].ptr + G)
    d_rec = ctx.to_device(rec) if len(rec) else None
    d_X = ctx.to_device(X) if n_map else None; d_cov = ctx.to_device(cv) if cv is not None and n_map else None
    st = lib().lvk_map_gather_obs(ctx.h, _p(d_rec), nr, _p(d_X), _p(d_cov), n_map, _p(al), float(sigma), at("obs"), at("idx"), at("info"))
    if check:
        ctx.check(st)
    ctx.sync()
    raw = {k: ctx.to_host(bufs[k], np.uint8, (sizes[k] + 2 * G,)).copy() for k in sizes}
    body = lambda k: raw[k][G:G + sizes[k]]
    info = body("info").view(MAP_OBS_INFO)[0]
    n_ok = int(info["n_ok"]) if st == 0 else 0
    out = dict(info=info, obs=body("obs").view(LANDMARK_OBS)[:n_ok], idx=body("idx").view(np.int32)[:n_ok], **{k + "_raw": v for k, v in raw.items()})
    return out if check else (st, out)
