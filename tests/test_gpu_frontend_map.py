"""GPU: lvk_frontend_set_map / lvk_frontend_match_map on a rendered stream (tests/mask_replay.py's 301 x 203 cut).  The map is the tracks of
one frame lifted to 3D at arbitrary depths through the numpy camera model and taken into a map frame of its own, so that they project
back to known pixels; points behind the camera and beside the image are mixed in.

selection      match_map's index, cell and depth are the restatement's (tests/map_select_ref.py) byte for byte, its queries equal or adjacent
               float32 to the long-double judge's
matching       its match records equal match_landmarks' - the existing call, on the same handle - for the returned queries and the map's
               descriptors, byte for byte
no disturbance a run with set_map and match_map calls behind every frame publishes the bits of a run without them
refusals       no map set, before the first frame, n over the cap, too little room; the handle goes on
set_map        replaces the map and clears it
end to end     localize.map_obs into LarVio.add_landmark_obs: APPLIED, as tests/test_gpu_frontend_match.py does it for landmark_obs"""
import ctypes as C

import numpy as np
import pytest

from tests import map_select_cases as SC
from tests import map_select_ref as R
from tests import mask_replay as MR
from tests import orb_match_cases as MC

pytestmark = pytest.mark.gpu

R_WC = SC._rot(np.random.default_rng(77)); P_WC = np.array([1.5, -0.7, 0.4])
CC = np.diag([0.004, 0.004, 0.004, 0.02, 0.02, 0.02]) ** 2


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


def lifted_map(cfg, tracks, seed=1, extra=40):
    """the tracks' pixels lifted to 3D (depth 2 - 9 m) plus `extra` points behind the camera or beside the image, shuffled, in the map frame of
    SC.ALIGN -> (X, cov, desc, the pixel each point should land on or NaN)"""
    from larvio_amd import localize
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cfg["intrinsics"]
    px = tracks["pts"].astype(np.float64)
    d = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy], -1); xy = d.copy()
    for _ in range(100):
        xy = xy + (d - localize.distort(xy, cfg["distortion_model"], cfg["distortion"]))
    z = rng.uniform(2.0, 9.0, len(px))
    p_c = np.concatenate([np.column_stack([xy * z[:, None], z]), np.column_stack([rng.uniform(-1, 1, (extra, 2)), rng.uniform(-6.0, -1.0, extra)]),
                          np.column_stack([rng.uniform(3.0, 5.0, (extra, 2)) * 4.0, np.full(extra, 4.0)])])
    want = np.concatenate([px, np.full((2 * extra, 2), np.nan)])
    desc = np.concatenate([tracks["desc"], rng.integers(0, 256, (2 * extra, 32), dtype=np.uint8)])
    order = rng.permutation(len(p_c))
    A = rng.normal(size=(len(p_c), 3, 3)); cov = 0.01 ** 2 * (A @ A.transpose(0, 2, 1) + 0.3 * np.eye(3))
    return SC._to_map(p_c[order], R_WC, P_WC, SC.ALIGN), cov, desc[order], want[order]


def test_selection_is_the_restatements_and_matching_is_match_landmarks(gpu_ctx, stream):
    from larvio_amd import ops
    from larvio_amd._lib import MATCH_OK
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 13)
    tr = gpu.tracks()
    assert gpu.state == 3 and len(tr["ids"]) > 20
    X, cov, desc, want_px = lifted_map(cfg, tr)
    gpu.set_map(X, cov, desc)
    assert gpu.map_size == len(X)
    for opt in (dict(), dict(rows=3, cols=4, quota=4, margin=6.0, r_min=5.0, r_max=25.0, max_depth=8.0)):
        o = R.options(**opt)
        rec, info = gpu.match_map(R_WC, P_WC, align=SC.ALIGN, cov_cam=CC, select=ops.map_select_options(**opt))
        ref = R.run(X, cov, desc, cfg, SC.ALIGN, R_WC, P_WC, CC, o); j = R.judge(X, cov, cfg, SC.ALIGN, R_WC, P_WC, CC, o)
        assert not SC.too_close(j, cfg, o).any()
        for f in ("n_selected", "n_visible", "n_behind", "n_far", "n_outside"):
            assert info[f] == ref["info"][f], f
        assert info["n_candidates"] > 100 and len(rec) == info["n_selected"] > 10
        for f in ("index", "cell", "depth"):
            assert rec[f].tobytes() == ref["sel"][f].tobytes(), f
        idx = rec["index"]
        for f in ("x", "y", "radius"):
            assert R.adjacent_or_equal(rec["q"][f], j[f][idx]).all(), f
        assert not rec["q"]["pad"].any() and not rec["pad"].any()
        assert np.abs(np.stack([rec["q"]["x"], rec["q"]["y"]], -1) - want_px[idx]).max() < 1e-3          # the lifted tracks land on their own pixels
        m2 = gpu.match_landmarks(np.stack([rec["q"]["x"], rec["q"]["y"]], -1), rec["q"]["radius"], desc[idx])
        assert gpu.last_match_candidates == info["n_candidates"]
        assert np.ascontiguousarray(rec["m"]).tobytes() == m2.tobytes()
        ok = rec["m"]["status"] == MATCH_OK
        assert (np.abs(rec["m"]["px"][ok] - want_px[idx][ok]).max(1) < 3.0).sum() >= 5                        # tracked corners are found at their own place
    gpu.close()


def test_map_calls_do_not_disturb_the_run(gpu_ctx, stream):
    frames, seq, cfg = stream

    def run(with_calls):
        gpu = _frontend(gpu_ctx, cfg)
        seen = []; held = []

        def after(i, img):
            if with_calls:
                t = gpu.tracks()
                if len(t["ids"]):
                    X, cov, desc, _ = lifted_map(cfg, t, seed=i, extra=5)
                    gpu.set_map(X, cov if i % 2 else None, desc)
                    rec, info = gpu.match_map(R_WC, P_WC, align=SC.ALIGN, cov_cam=CC if i % 3 else None)
                    seen.append(int(info["n_selected"]))
            t = gpu.tracks()
            held.append((t["ids"].tobytes(), t["pts"].tobytes(), t["lifetime"].tobytes(), t["init"].tobytes(), t["desc"].tobytes(), gpu.new_pts().tobytes()))
        msgs = MC.drive(_step(gpu), frames, seq, 10, after)
        gpu.close()
        return msgs, held, seen
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    assert sum(1 for m in a[0] if m) >= 3 and sum(b[2]) > 100          # messages were published, and the calls did select


def test_refusals_and_set_map_replaces_and_clears(gpu_ctx, stream):
    import larvio_amd
    from larvio_amd import ops
    from larvio_amd._lib import lib, _p
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)

    def status_of(f, *a, **kw):
        with pytest.raises(larvio_amd.LvkError) as e:
            f(*a, **kw)
        return int(str(e.value).split()[2].rstrip(":"))
    X = np.array([[0.0, 0.0, 4.0], [0.05, 0.05, 5.0], [0.0, 0.0, -4.0]]); desc = np.zeros((3, 32), np.uint8)
    I, z = np.eye(3), np.zeros(3)
    assert gpu.map_size == 0
    gpu.set_map(X, None, desc)                                           # a map may be set before the first frame ...
    assert gpu.map_size == 3
    assert status_of(gpu.match_map, I, z) == 1                           # ... but not looked up: LVK_ERR_ARG, no frame yet
    MC.drive(_step(gpu), frames, seq, 3)
    rec, info = gpu.match_map(I, z)
    assert info["n_selected"] == 2 and info["n_behind"] == 1 and dict(zip(rec["index"].tolist(), rec["depth"].tolist())) == {0: 4.0, 1: 5.0}
    gpu.set_map(X[::-1].copy(), None, desc)                              # replaced: the same points in another order
    rec2, _ = gpu.match_map(I, z)
    assert dict(zip(rec2["index"].tolist(), rec2["depth"].tolist())) == {1: 5.0, 2: 4.0}
    # refusals: n over the cap (refused before anything is read), a null pointer, bad options, too little room - and the map in force stays
    assert lib().lvk_frontend_set_map(gpu._h, _p(X), None, _p(desc), (1 << 20) + 1) == 3
    assert lib().lvk_frontend_set_map(gpu._h, _p(X), None, None, 3) == 1 and lib().lvk_frontend_set_map(gpu._h, None, None, _p(desc), 3) == 1
    assert lib().lvk_frontend_set_map(gpu._h, _p(X), None, _p(desc), -1) == 1
    assert gpu.map_size == 3
    assert status_of(gpu.match_map, I, z, select=ops.map_select_options(rows=17)) == 1
    assert status_of(gpu.match_map, np.full((3, 3), np.nan), z) == 1
    assert status_of(gpu.match_map, I, z, max_dist=257) == 1 and status_of(gpu.match_map, I, z, max_candidates=4097) == 3
    out = np.zeros(8, larvio_amd._lib.MAP_MATCH); n = C.c_int(0)
    assert lib().lvk_frontend_match_map(gpu._h, None, _p(np.eye(3).reshape(9)), _p(z), None, None, None, _p(out), 8, C.byref(n), None) == 3      # 1020 could be selected
    small = ops.map_select_options(rows=2, cols=2, quota=2)
    assert lib().lvk_frontend_match_map(gpu._h, None, _p(np.eye(3).reshape(9)), _p(z), None, C.byref(small), None, _p(out), 8, C.byref(n), None) == 0 and n.value == 2
    assert gpu.match_map(I, z)[0].tobytes() == rec2.tobytes()            # the handle goes on
    gpu.set_map(None, None, None)                                        # cleared
    assert gpu.map_size == 0 and status_of(gpu.match_map, I, z) == 1
    MC.drive(_step(gpu), frames[3:], seq, 3)
    assert gpu.state == 3
    gpu.close()


# ---------------------------------------------------------------- end to end: the selected and matched map points into the filter
def test_map_observations_are_applied_and_shrink_the_position_block(gpu_ctx):
    """As tests/test_gpu_frontend_match.py stages it: the filter runs on simulated messages; behind every message the map - known world points,
    held in a map frame of their own - is projected from a pose 2 cm and 0.3 degrees off by the stage entry, its queries are matched
    against corners staged at the true projections, and localize.map_obs turns the OK records into the batch.  The staged corners sit on whole
    pixels: a rounding error uniform in +-0.5 px against sigma = 1 px gives E[d^2] = 2 / 12 = 0.17 per observation, above the filter's default
    gate of 0.1026 (its 5 % quantile) two times out of three, so the filter is given the usual 99.9 % gate the header names."""
    import larvio_amd
    from larvio_amd import localize, ops, synthetic as S
    from larvio_amd._lib import MAP_MATCH, ALIGN_RESULT
    from tests import feature_sim
    from tests.test_gpu_landmark_fixes import _drive, _true_landmarks
    sim = feature_sim.simulate(4, t1=4.0, sw_size=10, fresh_ids=True)
    fcfg = S.frontend_config()
    tr = sim["traj"]
    rng = np.random.default_rng(20261101)
    res = np.zeros(1, ALIGN_RESULT)[0]; res["c"], res["s"], res["t"] = SC.ALIGN
    c_, s_, t_ = SC.ALIGN; Rz = np.array([[c_, -s_, 0.0], [s_, c_, 0.0], [0.0, 0.0, 1.0]])
    used = []

    def after(gpu, k, s):
        c = s["clones"][-1]; t = float(c["time"])
        p_w, _ = _true_landmarks(sim, rng, t, 12)
        X_map = (p_w - np.asarray(t_)) @ Rz                                          # the map's own frame
        cov_map = np.tile(1e-4 * np.eye(3), (len(X_map), 1, 1))
        R_wc = tr.R_wb(t) @ tr.R_cb.T; p_wc = tr.p_wb(t) - R_wc @ tr.t_cb
        true_px, ok = localize.predict_pixels(p_w, R_wc, p_wc, fcfg)
        assert ok.all()
        map_desc = rng.integers(0, 256, (len(p_w), 32), dtype=np.uint8)
        seen = map_desc.copy(); seen[:, 0] ^= 0x15                                   # three bits off
        cand_pts = np.concatenate([np.rint(true_px), rng.uniform(20, 400, (40, 2))]).astype(np.float32)
        cand_desc = np.concatenate([seen, rng.integers(0, 256, (40, 32), dtype=np.uint8)])
        a = 0.005; dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        sel = ops.map_select_queries(gpu_ctx, X_map, cov_map, map_desc, fcfg, R_wc @ dR, p_wc + 0.02, align=res, cov_cam=np.diag([0.006] * 3 + [0.03] * 3) ** 2,
                                     options=ops.map_select_options(max_r2=localize.view_limit(fcfg)))
        assert sel["info"]["n_selected"] == len(p_w)
        r = ops.orb_match_guided(gpu_ctx, cand_pts, cand_desc, np.stack([sel["q"]["x"], sel["q"]["y"]], -1), sel["q"]["radius"], sel["q_desc"])
        rec = np.zeros(len(r), MAP_MATCH)
        rec["index"] = sel["sel"]["index"]; rec["cell"] = sel["sel"]["cell"]; rec["q"] = sel["q"]; rec["depth"] = sel["sel"]["depth"]
        for f in ("status", "dist", "second", "n_window"):
            rec["m"][f] = r[f]
        rec["m"]["px"] = cand_pts[np.maximum(r["cand"], 0)]
        rec["m"]["und"] = ops.undistort(gpu_ctx, rec["m"]["px"], fcfg["intrinsics"], fcfg["distortion_model"], fcfg["distortion"], (1.0, 1.0, 0.0, 0.0))
        obs, idx = localize.map_obs(rec, X_map, cov_map, res, 1.0, fcfg)
        assert np.abs(obs["p_w"] - p_w[rec["index"][idx]]).max() < 1e-9
        used.append(len(idx))
        gpu.add_landmark_obs(obs["p_w"], obs["uv"], obs["sigma"], obs["cov_w"].reshape(-1, 3, 3), clone_id=int(c["id"]), tag=k)
    plain = _drive(gpu_ctx, sim)[0]
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after, setup=lambda gpu: gpu.set_landmark_options(13.816 / 0.1026, 0.1))
    rep = np.concatenate(reports)
    assert min(used) >= 8, used
    assert len(rep) == len(snaps) - 1 and np.all(rep["status"] == larvio_amd.larvio.LANDMARKS_APPLIED) and np.all(rep["n_used"] > 0), rep
    trace = lambda s: float(np.trace(s["P"][6:9, 6:9]))
    print("position block trace with map observations %.3g, without %.3g; used %d of %d" % (trace(snaps[-1]), trace(plain[-1]), stats["used"], stats["obs"]))
    assert trace(snaps[-1]) < trace(plain[-1])
