"""Plain restatements of what the frame path's three kernels compute (larvio_amd/csrc/fe_frame.hip), in numpy over the CPU oracle's own
stage functions (oracle/lvo.py): track_ref = k_fe_lk_both / k_fe_lk_pipe, commit_ref = k_fe_ransac_commit, msg_ref = k_fe_msg.  They are
checked on their own by tests/test_fe_frame_ref.py (hand cases, and the oracle's frame loop) and are the reference of
tests/test_gpu_frame_stages.py.  Outputs a kernel does not produce keep the caller's fill byte, as the stage entries leave them."""
import numpy as np
from oracle import lvo

ST_ALIVE, ST_FWD, ST_REV, ST_ORB = 0, 1, 2, 3
FM_THREADS, FM_THREADS_WIDE, FM_WIDE_FROM, FM_MAX_N = 256, 512, 512, 4096
ORB_MAX_DIST = 58
UNIT = (1.0, 1.0, 0.0, 0.0)


def filled(shape, dtype, fill):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = fill
    return a


def _inside(p, w, h):
    """the reference's in-image test, negated: !(y < 0 || y > h - 1 || x < 0 || x > w - 1)"""
    return ~((p[:, 1] < 0) | (p[:, 1] > h - 1) | (p[:, 0] < 0) | (p[:, 0] > w - 1))


def track_ref(prev, nxt, prev_planes, next_planes, pts, is_new, stored_desc, H, cam, w, h, grid=None, fill=0xA5, max_iter=30, eps=0.01):
    """One track set through forward LK, the in-image test, reverse LK, the round-trip test, the descriptor gate and the undistortion.
    prev / nxt: lvo.LkPyramid; *_planes: their orb_prepare() pairs; cam = (model, intr, dist).
    -> dict(curr (grid, 2), status (grid,), und (grid, 2, 2), desc (grid, 32) or None, point_levels, iterations)"""
    pts = lvo.pts(pts); n = len(pts)
    grid = n if grid is None else grid
    model, intr, dist = cam
    out = dict(curr=filled((grid, 2), np.float32, fill), status=filled(grid, np.uint8, fill), und=filled((grid, 2, 2), np.float32, fill),
               desc=filled((grid, 32), np.uint8, fill) if is_new else None, point_levels=0, iterations=0)
    if n == 0:
        return out
    nl = min(prev.n_levels, nxt.n_levels)
    start = lvo.apply_homography(np.asarray(H, np.float32).reshape(3, 3), pts)
    fwd, st, it = lvo.lk_track(prev, nxt, pts, start, max_iter, eps)
    ok = (st != 0) & _inside(fwd, w, h)                                     # fe_lk_forward_done
    code = np.full(n, ST_FWD, np.uint8)
    iters = int(it.sum()); levels = n * nl
    idx = np.flatnonzero(ok)
    if len(idx):
        back, sr, it2 = lvo.lk_track(nxt, prev, fwd[idx], pts[idx], max_iter, eps)
        iters += int(it2.sum()); levels += len(idx) * nl
        good = (sr != 0) & _inside(back, w, h)                              # fe_lk_round_trip
        dx = back[:, 0] - pts[idx, 0]; dy = back[:, 1] - pts[idx, 1]       # float32 differences
        dis = np.sqrt(dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64)).astype(np.float32)   # cv::norm is double, the result a float
        good &= ~(dis > 1)
        code[idx] = np.where(good, ST_ALIVE, ST_REV)
        dcur, _ = lvo.orb_describe(next_planes[0], next_planes[1], fwd[idx])
    dprev = None
    if is_new:
        dprev, _ = lvo.orb_describe(prev_planes[0], prev_planes[1], pts)
        out["desc"][:n] = dprev
    for k, i in enumerate(idx):                                             # fe_lk_finish: the gate only turns an alive point
        against = dprev[i] if is_new else stored_desc[i]
        if code[i] == ST_ALIVE and lvo.hamming(dcur[k], against) > ORB_MAX_DIST:
            code[i] = ST_ORB
    out["curr"][:n] = fwd                                                   # the forward result, whatever became of the point
    out["status"][:n] = code
    out["und"][:n, 0] = lvo.undistort(pts, intr, model, dist, intr)
    if len(idx):
        out["und"][idx, 1] = lvo.undistort(fwd[idx], intr, model, dist, intr)    # only behind a forward pass that succeeded
    out["point_levels"] = levels; out["iterations"] = iters
    return out


def mask_method(m):
    """cv::findFundamentalMat's dispatch on the point count"""
    return "none" if m < 7 else "seven" if m == 7 else "lmeds" if m < 15 else "ransac"


def commit_ref(mode, cap, src, dst, state):
    """k_fe_ransac_commit.  src: dict(pts, curr, status, und (n, 2, 2), desc (n, 32); mode 0: id, init, life); dst: dict(id, pts, ppts, init,
    life, desc) of cap slots; state: dict(next_id, dst_n, n_new, boot_ok).  Nothing is changed in place.
    -> (dst, state, branch): branch = dict(width, m, method, clipped, fail, kept, scratch): the workgroup width, the alive count, the mask
    method run (None when a failure rule came first), did the append stop at cap, the failure rules that fired (a tuple of 'cnt0', 'cnt1',
    'm', 'kept'), the mask's survivors, and `scratch`: leading slots of dst whose content is unspecified (a bootstrap that fails BEHIND
    the mask has already written its survivors; the set's count is 0, so nothing reads them)."""
    status = np.asarray(src["status"], np.uint8)
    n = min(len(status), cap)
    status = status[:n]
    dst = {k: np.array(v, copy=True) for k, v in dst.items()}
    state = dict(state)
    cnt0 = int((status != ST_FWD).sum()); cnt1 = int(((status != ST_FWD) & (status != ST_REV)).sum())
    alive = np.flatnonzero(status == ST_ALIVE); m = len(alive)
    fail = []
    if mode == 2:
        fail = [k for k, v in (("cnt0", cnt0), ("cnt1", cnt1), ("m", m)) if v < 20]
    elif mode == 1 and m < 20:
        fail = ["m"]
    br = dict(width=FM_THREADS_WIDE if cap > FM_WIDE_FROM else FM_THREADS, m=m, method=None, clipped=False, fail=(), kept=0, scratch=0)
    kept = np.zeros(0, np.int64)
    if not fail:
        keep = np.ones(m, bool)
        if m > 0:
            br["method"] = mask_method(m)
            und = np.asarray(src["und"], np.float32).reshape(-1, 2, 2)
            mask = lvo.find_fundamental_mask(und[alive, 0], und[alive, 1], 1.0, 0.99)
            assert (mask is None) == (m < 7)
            if mask is not None:
                keep = mask != 0
        kept = alive[keep]
        base = state["dst_n"] if mode == 1 else 0
        for r, i in enumerate(kept):
            d = base + r
            if d >= cap:
                br["clipped"] = True
                continue
            dst["pts"][d] = src["curr"][i]; dst["ppts"][d] = src["pts"][i]; dst["desc"][d] = src["desc"][i]
            if mode == 0:
                dst["id"][d] = src["id"][i]; dst["life"][d] = src["life"][i] + 1; dst["init"][d] = src["init"][i]
            else:
                dst["id"][d] = state["next_id"] + r; dst["life"][d] = 2
                dst["init"][d] = src["pts"][i] if mode == 1 else (-1.0, -1.0)
        if mode == 2 and len(kept) < 20:
            fail.append("kept"); br["scratch"] = len(kept)
        if mode == 1 and len(kept) <= 0:
            fail.append("kept")
    br["kept"] = len(kept); br["fail"] = tuple(fail)
    if mode == 0:
        state["dst_n"] = len(kept)
    elif mode == 1:
        if not fail:
            state["dst_n"] = min(state["dst_n"] + len(kept), cap); state["next_id"] += len(kept); state["n_new"] = 0
    else:
        state["boot_ok"] = 0 if fail else 1
        if not fail:
            state["dst_n"] = len(kept); state["next_id"] += len(kept); state["n_new"] = 0
        else:
            state["dst_n"] = 0
    return dst, state, br


def msg_ref(tset, cap, n, cam, dt_1, dt_2, prev_is_last, state, fill=0xA5):
    """k_fe_msg / getFeatureMsg as fe_msg_one has it: tset = dict(id, pts, ppts, init) of cap slots.  -> (message (cap,) OBS, init after the call, state)"""
    model, intr, dist = cam
    out = filled(cap, lvo.OBS, fill)
    init = np.array(tset["init"], np.float32, copy=True)
    state = dict(state)
    state["n_msg"] = n; state["n_host"] = n; state["msg_features"] += n; state["msg_count"] += 1
    if n == 0:
        return out, init, state
    uc = lvo.undistort(tset["pts"][:n], intr, model, dist, UNIT)        # float32 points: their differences are float32 differences
    ui = lvo.undistort(init[:n], intr, model, dist, UNIT)               # (cv::Point2f - cv::Point2f), only the division is double
    up = lvo.undistort(tset["ppts"][:n], intr, model, dist, UNIT)
    for i in range(n):
        f = np.zeros((), lvo.OBS)
        f["id"] = tset["id"][i]
        f["u"], f["v"] = float(uc[i, 0]), float(uc[i, 1])
        f["u_vel"] = float(uc[i, 0] - up[i, 0]) / dt_1; f["v_vel"] = float(uc[i, 1] - up[i, 1]) / dt_1
        if init[i, 0] == -1 and init[i, 1] == -1:
            f["u_init"] = -1; f["v_init"] = -1
        else:
            f["u_init"], f["v_init"] = float(ui[i, 0]), float(ui[i, 1])
            init[i] = (-1, -1)
            a = uc[i] if prev_is_last else up[i]
            f["u_init_vel"] = float(a[0] - ui[i, 0]) / dt_2; f["v_init_vel"] = float(a[1] - ui[i, 1]) / dt_2
        out[i] = f
    return out, init, state
