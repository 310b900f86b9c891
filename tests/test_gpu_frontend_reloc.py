"""GPU: lvk_frontend_relocalise_map (ImageProcessor.relocalise_map) on a rendered stream (tests/mask_replay.py's 301 x 203 cut).  The map's
true members are the frame's own corners (tests/orb_match_ref.frame_candidates) lifted to 3D at arbitrary depths and taken into a map frame
of their own, three bits of every descriptor inverted and a quarter of the descriptors swapped among themselves, which makes wrong matches;
the rest of the map is uniformly random descriptors at random positions.

same bits      the call equals the chain built by hand - frame_candidates, ops.orb_match_global, ops.align_draw_pairs,
               ops.align_ransac_2pt - bit for bit, with every pair, with drawn pairs and with a seed of the caller's
no disturbance a run of ten frames with a call behind every frame publishes the bits of a run without
refusals       no map, before the first frame, too little room; the handle goes on
end to end     a 20,000-point map yawed by 0.7 rad and shifted by metres: ALIGN_OK, then match_map with that alignment finds the true points
               again inside R_PX pixels"""
import ctypes as C

import numpy as np
import pytest

from tests import align_cases as AC
from tests import align_ref as AR
from tests import map_select_cases as SC
from tests import mask_replay as MR
from tests import orb_global_ref as GR
from tests import orb_match_cases as MC
from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu

# The end-to-end staging: every true member of the map is lifted from its corner moved by up to NOISE_PX in x and y, and the alignment's
# inlier threshold is THRESH in normalised units.  R_PX, the search radius of match_map behind the relocalisation, is the smallest of 2, 3,
# 4, 6, 8 px at which the long-double restatement passes on the same matches.  Measured worst pixel error of an inlier against its corner:
# restatement 0.709 px, library 0.709 px (248 inliers of 349 matches, the best counts 248, 247, 247); 2 px holds.
NOISE_PX, THRESH = 0.5, 0.0015
R_PX = 2.0
R_WC = SC._rot(np.random.default_rng(77)); P_WC = np.array([1.5, -0.7, 0.4])
PSI, SHIFT = 0.7, np.array([4.0, -3.0, 0.8])
UNIT = (1.0, 1.0, 0.0, 0.0)


def _frontend(gpu_ctx, cfg):
    import larvio_amd
    gpu = larvio_amd.ImageProcessor(cfg, gpu_ctx)
    assert gpu.initialize()
    return gpu


def _step(gpu):
    def f(img, ts, imu):
        have, msg = gpu.processImage(img, imu, ts=ts)
        return msg.features.tobytes() if have else b""
    return f


@pytest.fixture(scope="module")
def stream():
    return MR.sequence(MC.SEQ)


@pytest.fixture(scope="module")
def cands(stream):
    """the corners lvk_frontend_match_landmarks offers for frame 2 and their descriptors, computed once"""
    frames, seq, cfg = stream
    return R.frame_candidates(cfg, frames[2][1])


def staged_map(cfg, pts, desc, n_total, seed, noise_px=0.0):
    """-> (X (n_total, 3) in the map's own frame, descriptors, is_swapped (n_true,)): true member k is corner k of the frame, lifted from
    its pixel moved by up to noise_px in x and y (uniform: a map built from another session's observation of the point)"""
    from oracle import lvo
    rng = np.random.default_rng(seed)
    n = len(pts)
    seen = (pts + rng.uniform(-noise_px, noise_px, pts.shape)).astype(np.float32) if noise_px else pts
    und = lvo.undistort(seen, cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], UNIT).astype(np.float64)
    z = rng.uniform(2.0, 9.0, n)
    p_w = np.column_stack([und * z[:, None], z]) @ R_WC.T + P_WC
    X_true = (p_w - SHIFT) @ AC.rz(PSI)                                            # p_w = Rz X + shift
    d_true = desc.copy(); d_true[:, 0] ^= 0x15                                     # three bits off
    swapped = rng.permutation(n)[:n // 4]
    d_true[swapped] = d_true[np.roll(swapped, 1)]                                  # map point k now carries another point's descriptor
    is_swapped = np.zeros(n, bool); is_swapped[swapped] = True
    m = n_total - n
    X = np.concatenate([X_true, rng.uniform(-30.0, 30.0, (m, 3))])
    d = np.concatenate([d_true, rng.integers(0, 256, (m, 32), dtype=np.uint8)])
    return X, d, is_swapped


def _hand_chain(gpu_ctx, cfg, pts, desc, X, map_desc, max_matches, max_hypotheses, seed, match_kw, align_kw):
    from larvio_amd import ops
    from larvio_amd._lib import ALIGN_MATCH
    g = ops.orb_match_global(gpu_ctx, map_desc, desc, match_kw.get("max_dist", 58), match_kw.get("ratio_pct", 100), max_matches or 1024)
    sel = g["sel"]
    px = pts[sel["cand"]].astype(np.float32).reshape(-1, 2)
    und = ops.undistort(gpu_ctx, px, cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], UNIT).reshape(-1, 2) if len(sel) else np.zeros((0, 2), np.float32)
    am = np.zeros(len(sel), ALIGN_MATCH)
    am["X"] = X[sel["index"]]; am["u"] = und[:, 0].astype(np.float64); am["v"] = und[:, 1].astype(np.float64)
    pairs = ops.align_draw_pairs(len(sel), max_hypotheses, seed)
    want = ops.align_ransac_2pt(gpu_ctx, am, pairs, R_WC, P_WC, ops.align_options(**align_kw), want_hyp=False)
    return g, px, und, am, pairs, want


def test_call_is_the_chain_built_by_hand(gpu_ctx, stream, cands):
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    pts, desc = cands
    X, md, _ = staged_map(cfg, pts, desc, 3000, seed=5)
    gpu.set_map(X, None, md)
    assert len(pts) > 150
    for kw in (dict(max_matches=60), dict(), dict(seed=11), dict(seed=3, max_hypotheses=500, max_matches=200), dict(max_matches=1)):
        mk = dict(ratio_pct=80); ak = dict(min_inliers=8)
        res, m, info = gpu.relocalise_map(R_WC, P_WC, **kw, **mk, **ak)
        g, px, und, am, pairs, want = _hand_chain(gpu_ctx, cfg, pts, desc, X, md, kw.get("max_matches", 0), kw.get("max_hypotheses", 0), kw.get("seed", 0), mk, ak)
        assert info.tobytes() == g["info"].tobytes() and len(m) == info["n_selected"] == len(g["sel"]), (kw, info, g["info"])
        for f in ("cand", "index", "dist", "second"):
            assert np.array_equal(m[f], g["sel"][f]), (kw, f)
        assert m["px"].tobytes() == px.tobytes() and m["und"].tobytes() == und.tobytes(), kw       # the corner set is frame_candidates'
        assert res.tobytes() == want["result"].tobytes(), (kw, res, want["result"])
        assert np.array_equal(m["inlier"], want["mask"].astype(np.int32)) and not m["pad"].any(), kw
        if kw.get("max_matches") == 60:
            assert len(pairs) == 60 * 59 // 2 and res["status"] == AR.OK                         # every pair
        elif kw.get("max_matches") == 1:
            assert res["status"] == AR.NO_MODEL and len(m) == 1                                  # the stage entry's own rule, no error
        else:
            assert len(pairs) == kw.get("max_hypotheses", 4096) and res["status"] == AR.OK       # drawn pairs
    gpu.close()


def test_relocalisation_calls_do_not_disturb_the_run(gpu_ctx, stream):
    frames, seq, cfg = stream
    rng = np.random.default_rng(9)
    filler = rng.integers(0, 256, (2500, 32), dtype=np.uint8); Xf = rng.uniform(-20.0, 20.0, (3000, 3))

    def run(with_calls):
        gpu = _frontend(gpu_ctx, cfg)
        seen = []; held = []

        def after(i, img):
            if with_calls:
                t = gpu.tracks()
                d = np.concatenate([t["desc"], filler])[:3000] if len(t["ids"]) else filler
                gpu.set_map(Xf[:len(d)], None, d)
                res, m, info = gpu.relocalise_map(R_WC, P_WC, seed=i + 1, ratio_pct=80)
                seen.append(int(info["n_ok"]))
            t = gpu.tracks()
            held.append((t["ids"].tobytes(), t["pts"].tobytes(), t["lifetime"].tobytes(), t["init"].tobytes(), t["desc"].tobytes(), gpu.new_pts().tobytes()))
        msgs = MC.drive(_step(gpu), frames, seq, 10, after)
        gpu.close()
        return msgs, held, seen
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    assert sum(1 for m in a[0] if m) >= 3 and len(b[2]) == 10 and sum(b[2]) > 10          # messages were published, and the calls did match


def test_refusals(gpu_ctx, stream):
    import larvio_amd
    from larvio_amd._lib import lib, _p, ALIGN_RESULT, RELOC_MATCH
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)

    def status_of(**kw):
        with pytest.raises(larvio_amd.LvkError) as e:
            gpu.relocalise_map(R_WC, P_WC, **kw)
        return int(str(e.value).split()[2].rstrip(":"))
    rng = np.random.default_rng(2)
    X = rng.uniform(-5, 5, (500, 3)); d = rng.integers(0, 256, (500, 32), dtype=np.uint8)
    assert status_of() == 1                                                  # LVK_ERR_ARG: no map
    gpu.set_map(X, None, d)
    assert status_of() == 1                                                  # LVK_ERR_ARG: no frame yet
    MC.drive(_step(gpu), frames, seq, 3)
    good = gpu.relocalise_map(R_WC, P_WC, seed=4)
    res = np.zeros(1, ALIGN_RESULT); out = np.zeros(8, RELOC_MATCH); n = C.c_int(-7)
    raw = lambda mm, cap: lib().lvk_frontend_relocalise_map(gpu._h, _p(np.ascontiguousarray(R_WC).reshape(9)), _p(P_WC), None, None, mm, 0, 0, _p(res), _p(out), cap, C.byref(n), None)
    assert raw(0, 8) == 3 and raw(9, 8) == 3 and n.value == -7               # LVK_ERR_CAPACITY: room for 8, 1024 / 9 could be selected
    assert raw(8, 8) == 0 and 0 <= n.value <= 8
    assert status_of(max_matches=1025) == 1 and status_of(max_hypotheses=4097) == 3 and status_of(max_matches=-1) == 1
    assert status_of(max_dist=257) == 1 and status_of(max_candidates=4097) == 3 and status_of(thresh=float("nan")) == 1
    again = gpu.relocalise_map(R_WC, P_WC, seed=4)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, good))      # the handle goes on, and so does the stream
    gpu.set_map(None, None, None)
    assert status_of() == 1
    MC.drive(_step(gpu), frames[3:], seq, 3)
    assert gpu.state == 3
    gpu.close()


# ---------------------------------------------------------------- end to end: a 20,000-point map in its own frame, found and brought over
def test_a_20000_point_map_is_relocalised(gpu_ctx, stream, cands):
    """The capability: 20,000 points cannot be asked about through the guided matcher's 1024 queries without a pose to pick them by.  The
    true members (the frame's corners, a quarter of them carrying another member's descriptor) are 2 % of the map; each was lifted from its
    corner moved by up to NOISE_PX, and the RANSAC threshold THRESH (0.69 px at this focal length) is of the noise's size, so that no
    hypothesis collects every right match and the hypotheses' counts differ.  Before the GPU is relied on, the restatements alone
    (tests/orb_global_ref.py, tests/align_ref.py in long double) must give at least min_inliers OK matches, ALIGN_OK, a unique best inlier
    count, and the same discrete results in float64.  Then: ALIGN_OK with the restatement's mask, no wrong match among the inliers, and
    match_map with the alignment finds every inlier's map point again at its own corner inside R_PX.  Measured on an MI355X: 349 matches (87 wrong), best counts 248, 247, 247; worst pixel error of an inlier 0.709 px for both (see R_PX above); match_map selected 829 points and found 248 of 248 inliers again."""
    import larvio_amd
    from larvio_amd import localize, ops
    from larvio_amd._lib import MATCH_OK
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    pts, desc = cands
    n_true = len(pts)
    X, md, is_swapped = staged_map(cfg, pts, desc, 20000, seed=20261021, noise_px=NOISE_PX)
    opt = dict(min_inliers=12, thresh=THRESH)
    # ---- the inputs, judged on the CPU alone
    g = GR.match(md, desc, 58, 80, 1024)
    sel = g["sel"]
    from oracle import lvo
    und = lvo.undistort(pts[sel["cand"]], cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], UNIT).astype(np.float64)
    pairs = AR.draw_pairs(len(sel))
    ref = AR.run(X[sel["index"]], und, pairs, R_WC, P_WC, opt)
    ref64 = AR.run(X[sel["index"]], und, pairs, R_WC, P_WC, opt, kind="f64")
    wrong = sel["index"] != sel["cand"]
    counts = np.sort(ref["count"].ravel())
    print("restatement: %d corners, %d OK matches (%d wrong), best inlier counts %s" % (n_true, len(sel), int(wrong.sum()), counts[-3:].tolist()))
    assert len(sel) >= opt["min_inliers"] and wrong.any() and ref["status"] == AR.OK
    assert not ref["tie"] and counts[-1] > counts[-2]                              # a unique best inlier count
    assert not AR.same_discrete(ref, ref64)                                        # and nothing discrete hangs on rounding
    # ---- the library
    gpu.set_map(X, None, md)
    res, m, info = gpu.relocalise_map(R_WC, P_WC, ratio_pct=80, **opt)
    assert res["status"] == AR.OK and info["n_selected"] == len(sel) and np.array_equal(m["index"], sel["index"]) and np.array_equal(m["cand"], sel["cand"])
    assert np.array_equal(m["inlier"], ref["mask"].astype(np.int32)) and res["n_inliers"] == ref["n_inliers"]
    inl = m["inlier"].astype(bool)
    assert (m["index"][inl] == m["cand"][inl]).all() and not is_swapped[m["index"][inl]].any()     # every inlier is a right match of an unswapped member

    def worst_px(c, s, tt):
        rec = np.zeros(1, larvio_amd._lib.ALIGN_RESULT)[0]; rec["c"] = float(c); rec["s"] = float(s); rec["t"] = np.asarray(tt, np.float64)
        p_al, _ = localize.apply_alignment(rec, X[m["index"][inl]])
        px, okp = localize.predict_pixels(p_al, R_WC, P_WC, cfg)
        assert okp.all()
        return float(np.linalg.norm(px.astype(np.float64) - m["px"][inl], axis=1).max())
    e_ref = worst_px(*ref["model"]); e_gpu = worst_px(res["c"], res["s"], res["t"])
    print("worst pixel error of an inlier against its corner: restatement %.4f px, library %.4f px; %d inliers of %d matches" % (e_ref, e_gpu, int(inl.sum()), len(m)))
    assert e_ref <= R_PX and e_gpu <= R_PX
    err = np.abs(np.arctan2(float(res["s"]), float(res["c"])) - PSI), np.abs(res["t"] - SHIFT).max()
    print("alignment error: yaw %.2e rad, translation %.2e m" % err)
    assert err[0] < 1e-3 and err[1] < 1e-2
    # ---- the per-frame link takes over: the aligned map, selected and matched inside R_PX
    rec, minfo = gpu.match_map(R_WC, P_WC, align=res, select=ops.map_select_options(r_min=R_PX, r_max=R_PX, max_r2=localize.view_limit(cfg)))
    by_index = {int(r["index"]): r for r in rec}
    found = [i for i in m["index"][inl] if int(i) in by_index and by_index[int(i)]["m"]["status"] == MATCH_OK and np.array_equal(by_index[int(i)]["m"]["px"], pts[i])]
    print("match_map: %d selected, %d of %d inliers found again at their own corner" % (minfo["n_selected"], len(found), int(inl.sum())))
    assert len(found) == int(inl.sum())
    gpu.close()
