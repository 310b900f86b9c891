"""Guided ORB matching (lvk_orb_match_guided, lvk_frontend_match_landmarks) restated in plain numpy from the contract in include/lvk_c.h.
There is no reference counterpart, so this restatement is the judge of the GPU tests; tests/test_orb_match_ref.py holds it to a
brute-force double loop over oracle.lvo.hamming first.

    window   candidate c is in the window of query q iff dx = cx - qx; dy = cy - qy; dx*dx + dy*dy <= radius*radius, every step float32
             (numpy rounds each float32 operation on its own: no contraction); a NaN anywhere makes the comparison false
    best     smallest Hamming distance in the window, ties to the lowest candidate index; second = smallest distance over the others, -1
    status   NO_CANDIDATE (n_window == 0; cand = dist = second = -1), TOO_FAR (dist > max_dist), AMBIGUOUS (second >= 0 and
             100 dist > ratio_pct second), else provisional; per claimed candidate the smallest (dist, query) is OK, the rest CONFLICT"""
import numpy as np

OK, NO_CANDIDATE, TOO_FAR, AMBIGUOUS, CONFLICT = 0, 1, 2, 3, 4
RESULT = np.dtype([("cand", np.int32), ("dist", np.int32), ("second", np.int32), ("n_window", np.int32), ("status", np.int32), ("pad", np.int32)])
LANDMARK_MATCH = np.dtype([("status", np.int32), ("dist", np.int32), ("second", np.int32), ("n_window", np.int32), ("px", np.float32, 2), ("und", np.float32, 2)])
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming_rows(cand_desc, q_desc):
    """distances of one 32-byte descriptor to every row of cand_desc (k, 32)"""
    return _POP[np.bitwise_xor(cand_desc, q_desc[None, :])].sum(1, dtype=np.int32)


def in_window(cand_pts, qx, qy, radius):
    cp = np.asarray(cand_pts, np.float32).reshape(-1, 2)
    qx, qy, radius = np.float32(qx), np.float32(qy), np.float32(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = cp[:, 0] - qx; dy = cp[:, 1] - qy
        return dx * dx + dy * dy <= radius * radius


def match(cand_pts, cand_desc, q_px, q_radius, q_desc, max_dist=58, ratio_pct=100):
    """-> RESULT array, one record per query"""
    cp = np.asarray(cand_pts, np.float32).reshape(-1, 2); cd = np.asarray(cand_desc, np.uint8).reshape(-1, 32)
    qp = np.asarray(q_px, np.float32).reshape(-1, 2); qd = np.asarray(q_desc, np.uint8).reshape(-1, 32)
    rad = np.broadcast_to(np.asarray(q_radius, np.float32), (len(qp),))
    out = np.zeros(len(qp), RESULT)
    for q in range(len(qp)):
        idx = np.nonzero(in_window(cp, qp[q, 0], qp[q, 1], rad[q]))[0]
        r = out[q]
        r["n_window"] = len(idx)
        if len(idx) == 0:
            r["cand"] = r["dist"] = r["second"] = -1; r["status"] = NO_CANDIDATE
            continue
        d = hamming_rows(cd[idx], qd[q])
        b = int(np.argmin(d))                                # the first minimum: idx ascends, so the lowest candidate index
        others = np.delete(d, b)
        r["cand"] = idx[b]; r["dist"] = d[b]; r["second"] = others.min() if len(others) else -1
        if r["dist"] > max_dist:
            r["status"] = TOO_FAR
        elif r["second"] >= 0 and 100 * int(r["dist"]) > ratio_pct * int(r["second"]):
            r["status"] = AMBIGUOUS
        else:
            r["status"] = OK                                 # provisional
    prov = np.nonzero(out["status"] == OK)[0]
    for c in np.unique(out["cand"][prov]):
        claim = prov[out["cand"][prov] == c]
        win = min(claim, key=lambda q: (int(out["dist"][q]), int(q)))
        out["status"][claim[claim != win]] = CONFLICT
    return out


def frame_candidates(cfg, img, max_candidates=4096, quality=0.01, min_distance=None):
    """the corners lvk_frontend_match_landmarks offers for a frame and their descriptors, on the oracle's planes of that frame: CLAHE as
    configured, the LK pyramid's level 0, its min-eigenvalue map, the selection without any mask, the ORB planes' descriptors"""
    from oracle import lvo
    from tests import gftt_ref
    det = lvo.clahe(img) if cfg["flag_equalize"] else np.ascontiguousarray(img, np.uint8)
    pyr = lvo.LkPyramid(det, cfg["patch_size"], cfg["pyramid_levels"])
    md = float(cfg["min_distance"] if min_distance is None else min_distance)
    pts = gftt_ref.select(pyr.min_eigen_map(), max_candidates, quality, md)
    ext, blur = pyr.orb_prepare()
    desc, _ = lvo.orb_describe(ext, blur, pts)
    return pts, desc


def frontend_match(cfg, img, q_px, q_radius, q_desc, max_candidates=4096, quality=0.01, min_distance=None, max_dist=58, ratio_pct=100, cands=None):
    """lvk_frontend_match_landmarks on frame `img` -> (LANDMARK_MATCH array, number of candidates); cands: frame_candidates() of the frame,
    when the caller already has them"""
    from oracle import lvo
    pts, desc = cands if cands is not None else frame_candidates(cfg, img, max_candidates, quality, min_distance)
    r = match(pts, desc, q_px, q_radius, q_desc, max_dist, ratio_pct)
    out = np.zeros(len(r), LANDMARK_MATCH)
    for k in ("status", "dist", "second", "n_window"):
        out[k] = r[k]
    has = r["cand"] >= 0
    if has.any():
        out["px"][has] = pts[r["cand"][has]]
        out["und"][has] = lvo.undistort(out["px"][has], cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], (1.0, 1.0, 0.0, 0.0))
    return out, len(pts)


# ---------------------------------------------------------------- hand-made descriptors
def desc_with_bits(k, start=0):
    """a 32-byte descriptor with exactly k bits set, from bit `start` on (wrapping): its distance to the zero descriptor is k"""
    bits = np.zeros(256, np.uint8)
    bits[(start + np.arange(k)) % 256] = 1
    return np.packbits(bits)
