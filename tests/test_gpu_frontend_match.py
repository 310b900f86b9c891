"""GPU: lvk_frontend_match_landmarks on a rendered stream (tests/mask_replay.py's 301 x 203 cut, two pyramid levels).

chain         after frame k the call's records are the restatement's (tests/orb_match_ref.py) on the oracle's planes of that frame, byte for
              byte, und included - with the defaults and with every option set
tracking      the map is the tracks of frame 20; at frame 25 the survivors are looked up from their own pixels shifted by (+3, -2), radius 8
no disturbance a run with a match call behind every frame publishes the bits of a run without
refusals      before the first frame; the selection's LVK_ERR_CAPACITY at min_distance 1 passes through and the handle goes on
end to end    matched corners of known points, through larvio_amd.localize, into LarVio.add_landmark_obs: APPLIED, and the position block shrinks"""
import numpy as np
import pytest

from tests import mask_replay as MR
from tests import orb_match_cases as MC
from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu


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


def test_chain_equals_the_restatement_on_the_oracles_planes(gpu_ctx, stream):
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    k = 12
    MC.drive(_step(gpu), frames, seq, k + 1)
    tr = gpu.tracks()
    assert gpu.state == 3 and len(tr["ids"]) > 20
    rng = np.random.default_rng(3)
    q_px = np.concatenate([tr["pts"] + rng.uniform(-3, 3, tr["pts"].shape).astype(np.float32), [[np.nan, 5.0], [-40.0, -40.0]]]).astype(np.float32)
    desc = np.concatenate([tr["desc"], tr["desc"][:2]])
    rad = np.concatenate([np.full(len(tr["pts"]), 8.0), [8.0, 8.0]]).astype(np.float32); rad[::5] = 25.0
    img = frames[k][1]
    got = gpu.match_landmarks(q_px, rad, desc)
    want, n_cand = R.frontend_match(cfg, img, q_px, rad, desc)
    assert gpu.last_match_candidates == n_cand and n_cand > 100
    for f in want.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), (f, got[f][:6], want[f][:6])
    assert got.tobytes() == want.tobytes()
    assert (got["status"] == R.OK).sum() >= 5 and (got["status"][-2:] == R.NO_CANDIDATE).all() and (got["px"][-2:] == 0).all() and (got["und"][-2:] == 0).all()
    opts = dict(max_candidates=50, quality=0.05, min_distance=7.0, max_dist=40, ratio_pct=80)
    got = gpu.match_landmarks(q_px, rad, desc, **opts)
    want, n_cand = R.frontend_match(cfg, img, q_px, rad, desc, **opts)
    assert gpu.last_match_candidates == n_cand == 50 and got.tobytes() == want.tobytes()
    assert len(gpu.match_landmarks(np.zeros((0, 2)), 8.0, np.zeros((0, 32), np.uint8))) == 0 and gpu.last_match_candidates > 100
    gpu.close()


def test_tracking_map_points_are_found_again_five_frames_later(gpu_ctx, stream):
    """The oracle's figure (tests/test_orb_match_ref.py::test_oracle_tracking_share_is_the_recorded_figure): 41 survivors, 29 OK, 27 of
    them (93.1 %) within 2 px of the track's own position; the GPU front-end must reach that share minus 5 points."""
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    held = {}

    def after(i, img):
        if i == MC.TRACK_K:
            held["map"] = gpu.tracks()
    MC.drive(_step(gpu), frames, seq, MC.TRACK_K + MC.TRACK_AHEAD + 1, after)
    q, desc, own = MC.tracking_queries(held["map"], gpu.tracks())
    m = gpu.match_landmarks(q, MC.RADIUS, desc)
    n_ok, share = MC.near_share(m, own)
    print(f"{len(q)} queries, {gpu.last_match_candidates} corners, {n_ok} OK, share within {MC.NEAR} px {share:.4f} (oracle {MC.ORACLE_SHARE:.4f})")
    assert n_ok >= 1 and (m["dist"][m["status"] == R.OK] <= 58).all()
    assert share >= MC.ORACLE_SHARE - 0.05
    gpu.close()


def test_match_calls_do_not_disturb_the_run(gpu_ctx, stream):
    frames, seq, cfg = stream

    def run(with_calls):
        gpu = _frontend(gpu_ctx, cfg)
        seen = []

        def after(i, img):
            if with_calls:
                t = gpu.tracks()
                m = gpu.match_landmarks(t["pts"], 8.0, t["desc"]) if len(t["ids"]) else gpu.match_landmarks(np.full((3, 2), 50.0), 30.0, np.zeros((3, 32), np.uint8))
                seen.append(int((m["status"] == R.OK).sum()))
            t = gpu.tracks()
            held.append((t["ids"].tobytes(), t["pts"].tobytes(), t["lifetime"].tobytes(), t["init"].tobytes(), t["desc"].tobytes(), gpu.new_pts().tobytes()))
        held = []
        msgs = MC.drive(_step(gpu), frames, seq, 10, after)
        gpu.close()
        return msgs, held, seen
    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1] == b[1]
    assert sum(1 for m in a[0] if m) >= 3 and sum(b[2]) > 20          # messages were published, and the calls did match


def test_refusals(gpu_ctx, stream):
    import larvio_amd
    frames, seq, cfg = stream
    gpu = _frontend(gpu_ctx, cfg)
    q = np.full((4, 2), 60.0, np.float32); d = np.zeros((4, 32), np.uint8)

    def status_of(**kw):
        with pytest.raises(larvio_amd.LvkError) as e:
            gpu.match_landmarks(q, 8.0, d, **kw)
        return int(str(e.value).split()[2].rstrip(":"))
    assert status_of() == 1                                             # LVK_ERR_ARG: no frame yet
    MC.drive(_step(gpu), frames, seq, 3)
    good = gpu.match_landmarks(q, 8.0, d)
    assert status_of(min_distance=1.0) == 3                             # LVK_ERR_CAPACITY of the selection: 301 x 203 one-pixel cells
    assert status_of(max_candidates=4097) == 3
    assert status_of(max_dist=257) == 1 and status_of(ratio_pct=101) == 1 and status_of(quality=-0.5) == 1 and status_of(min_distance=float("nan")) == 1
    with pytest.raises(larvio_amd.LvkError):
        gpu.match_landmarks(np.zeros((1025, 2)), 8.0, np.zeros((1025, 32), np.uint8))
    assert gpu.match_landmarks(q, 8.0, d).tobytes() == good.tobytes()   # the handle goes on, and so does the stream
    MC.drive(_step(gpu), frames[3:], seq, 3)
    assert gpu.state == 3
    gpu.close()


# ---------------------------------------------------------------- end to end: matched corners into the filter
def test_matched_landmarks_are_applied_and_shrink_the_position_block(gpu_ctx):
    """The filter runs on the simulated messages of tests/test_gpu_landmark_fixes.py.  Behind every message a frame of the newest clone is
    staged for the matcher: known world points projected through the camera model to whole-pixel corners (plus distractors), each with its
    map descriptor a few bits off; the queries come from localize.predict_pixels at a pose 2 cm and 0.3 degrees off, the observations
    from the matcher's OK records through the library's undistortion and localize.landmark_obs."""
    import larvio_amd
    from larvio_amd import localize, ops, synthetic as S
    from tests import feature_sim
    from tests.test_gpu_landmark_fixes import _drive, _true_landmarks
    sim = feature_sim.simulate(4, t1=4.0, sw_size=10, fresh_ids=True)
    fcfg = S.frontend_config()
    tr = sim["traj"]
    rng = np.random.default_rng(20261023)
    used = []

    def after(gpu, k, s):
        c = s["clones"][-1]; t = float(c["time"])
        p_w, _ = _true_landmarks(sim, rng, t, 12)
        R_wc = tr.R_wb(t) @ tr.R_cb.T; p_wc = tr.p_wb(t) - R_wc @ tr.t_cb
        true_px, ok = localize.predict_pixels(p_w, R_wc, p_wc, fcfg)
        assert ok.all()
        map_desc = rng.integers(0, 256, (len(p_w), 32), dtype=np.uint8)
        seen = map_desc.copy(); seen[:, 0] ^= 0x15                                   # three bits off
        cand_pts = np.concatenate([np.rint(true_px), rng.uniform(20, 400, (40, 2))]).astype(np.float32)
        cand_desc = np.concatenate([seen, rng.integers(0, 256, (40, 32), dtype=np.uint8)])
        a = 0.005; dR = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        q_px, ok = localize.predict_pixels(p_w, R_wc @ dR, p_wc + 0.02, fcfg)
        r = ops.orb_match_guided(gpu_ctx, cand_pts, cand_desc, q_px, 25.0, map_desc)
        m = np.zeros(len(r), larvio_amd._lib.LANDMARK_MATCH)
        for f in ("status", "dist", "second", "n_window"):
            m[f] = r[f]
        m["px"] = cand_pts[np.maximum(r["cand"], 0)]
        m["und"] = ops.undistort(gpu_ctx, m["px"], fcfg["intrinsics"], fcfg["distortion_model"], fcfg["distortion"], (1.0, 1.0, 0.0, 0.0))
        obs, idx = localize.landmark_obs(m, p_w, None, 1.0, fcfg)
        used.append(len(idx))
        gpu.add_landmark_obs(obs["p_w"], obs["uv"], obs["sigma"], obs["cov_w"].reshape(-1, 3, 3), clone_id=int(c["id"]), tag=k)
    plain = _drive(gpu_ctx, sim)[0]
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after)
    rep = np.concatenate(reports)
    assert min(used) >= 8, used
    assert len(rep) == len(snaps) - 1 and np.all(rep["status"] == larvio_amd.larvio.LANDMARKS_APPLIED) and np.all(rep["n_used"] > 0), rep
    trace = lambda s: float(np.trace(s["P"][6:9, 6:9]))
    print("position block trace with matched landmarks %.3g, without %.3g; used %d of %d" % (trace(snaps[-1]), trace(plain[-1]), stats["used"], stats["obs"]))
    assert trace(snaps[-1]) < trace(plain[-1])
