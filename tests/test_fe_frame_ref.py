"""tests/fe_frame_ref.py held to account without a GPU: hand-made commit and message cases whose result can be written down, the frame
reference (track_ref -> commit_ref -> msg_ref) against the oracle's own frame loop, and the reference half of every case of
tests/test_gpu_frame_stages.py (tests/fe_frame_cases.py: the same tables) held to the branch it was built for."""
import numpy as np
import pytest
from oracle import lvo
from tests import fe_frame_ref as R
from tests import fe_frame_cases as K


def _src(n, status, seed=0, shift=(3.0, -2.0)):
    rng = np.random.default_rng(seed)
    p = rng.uniform(20, 300, (n, 2)).astype(np.float32)
    und = np.stack([p, p + np.float32(shift)], 1)              # a pure translation: every pair fits one epipolar geometry exactly
    return dict(pts=p, curr=(p + 1).astype(np.float32), status=np.asarray(status, np.uint8), und=und, desc=rng.integers(0, 256, (n, 32)).astype(np.uint8),
                id=np.arange(n, dtype=np.uint64) + 500, init=(p - 1).astype(np.float32), life=np.arange(n, dtype=np.int32) + 3)


def _dst(cap):
    return {k: R.filled(s, t, 0xA5) for k, (s, t) in dict(id=(cap, np.uint64), pts=((cap, 2), np.float32), ppts=((cap, 2), np.float32),
                                                        init=((cap, 2), np.float32), life=(cap, np.int32), desc=((cap, 32), np.uint8)).items()}


STATE = dict(next_id=77, dst_n=0, n_new=5, boot_ok=-1)


def test_commit_all_alive_translation_keeps_everything_in_order():
    n, cap = 40, 64
    s = _src(n, np.zeros(n))
    d, st, br = R.commit_ref(0, cap, s, _dst(cap), STATE)
    assert br == dict(width=256, m=n, method="ransac", clipped=False, fail=(), kept=n, scratch=0)
    assert st == dict(next_id=77, dst_n=n, n_new=5, boot_ok=-1)
    assert np.array_equal(d["id"][:n], s["id"]) and np.array_equal(d["life"][:n], s["life"] + 1) and np.array_equal(d["init"][:n], s["init"])
    assert np.array_equal(d["pts"][:n], s["curr"]) and np.array_equal(d["ppts"][:n], s["pts"]) and np.array_equal(d["desc"][:n], s["desc"])
    assert all((v[n:].view(np.uint8) == 0xA5).all() for v in d.values())


@pytest.mark.parametrize("m,method", [(0, None), (6, "none"), (7, "seven")])
def test_commit_small_sets_keep_everything(m, method):
    """fewer than 7 alive: no mask at all; exactly 7: a mask of ones.  Gross outliers among them stay"""
    n, cap = 12, 64
    status = np.array([R.ST_ALIVE if i % 2 == 0 and i // 2 < m else 1 + i % 3 for i in range(n + 4)], np.uint8)[:n + 4]
    s = _src(n + 4, status)
    s["und"][0, 1] += 90                                        # would be thrown out by any fitted model
    d, st, br = R.commit_ref(0, cap, s, _dst(cap), STATE)
    alive = np.flatnonzero(status == 0)
    assert len(alive) == m and br["m"] == m and br["method"] == method and br["kept"] == m and st["dst_n"] == m
    assert np.array_equal(d["id"][:m], s["id"][alive]) and np.array_equal(d["life"][:m], s["life"][alive] + 1)


def test_commit_clipped_append_and_unclipped_ids():
    n, cap = 30, 32
    s = _src(n, np.zeros(n)); s["id"] = s["init"] = s["life"] = None
    before = _dst(cap); before["id"][:10] = 1
    d, st, br = R.commit_ref(1, cap, s, before, dict(next_id=100, dst_n=10, n_new=n, boot_ok=0))
    assert br["clipped"] and br["kept"] == 30 and br["fail"] == ()
    assert st == dict(next_id=130, dst_n=32, n_new=0, boot_ok=0)               # ids run on for the eight that found no slot
    assert np.array_equal(d["id"][:10], before["id"][:10]) and np.array_equal(d["id"][10:], np.arange(100, 122, dtype=np.uint64))
    assert np.array_equal(d["init"][10:], s["pts"][:22]) and (d["life"][10:] == 2).all()


def test_commit_failure_rules():
    s = _src(30, [0] * 19 + [3] * 11); s["id"] = s["init"] = s["life"] = None
    st0 = dict(next_id=5, dst_n=4, n_new=30, boot_ok=1)
    d, st, br = R.commit_ref(1, 64, s, _dst(64), st0)
    assert br["fail"] == ("m",) and st == st0 and all((v.view(np.uint8) == 0xA5).all() for v in d.values())
    d, st, br = R.commit_ref(2, 64, s, _dst(64), st0)
    assert br["fail"] == ("m",) and st == dict(next_id=5, dst_n=0, n_new=30, boot_ok=0)
    s = _src(30, [0] * 20 + [1] * 10); s["id"] = s["init"] = s["life"] = None
    d, st, br = R.commit_ref(2, 64, s, _dst(64), st0)
    assert br["fail"] == () and st == dict(next_id=25, dst_n=20, n_new=0, boot_ok=1) and (d["init"][:20] == -1).all() and (d["life"][:20] == 2).all()
    assert np.array_equal(d["id"][:20], np.arange(5, 25, dtype=np.uint64))


def test_message_formulas_on_three_hand_computed_features():
    """an undistorted camera (no distortion): normalised coordinates are (x - cx) / fx, (y - cy) / fy of the float32 pixel"""
    cam = (0, (100.0, 200.0, 50.0, 40.0), (0.0, 0.0, 0.0, 0.0))
    ts = dict(id=np.array([9, 8, 7], np.uint64), pts=np.array([[150, 240], [50, 40], [0, 0]], np.float32), ppts=np.array([[100, 140], [60, 40], [25, 90]], np.float32),
              init=np.array([[-1, -1], [75, 90], [-1, 20]], np.float32))
    st0 = dict(n_msg=0, n_host=0, msg_features=10, msg_count=2)
    for prev_is_last in (0, 1):
        out, init, st = R.msg_ref(ts, 3, 3, cam, 0.5, 0.25, prev_is_last, st0)
        assert st == dict(n_msg=3, n_host=3, msg_features=13, msg_count=3)
        assert out["id"].tolist() == [9, 8, 7]
        f = lambda x: float(np.float32(x))                                        # undistorted points are float32 points
        assert out["u"].tolist() == [1.0, 0.0, -0.5] and out["v"].tolist() == [1.0, 0.0, f(-0.2)]
        assert out["u_vel"].tolist() == [1.0, (0.0 - f(0.1)) / 0.5, -0.5] and out["v_vel"].tolist() == [1.0, 0.0, f(f(-0.2) - 0.25) / 0.5]
        assert out["u_init"].tolist() == [-1.0, 0.25, f(-0.51)] and out["v_init"].tolist() == [-1.0, 0.25, f(-0.1)]
        want_u = [0.0, (0.0 - 0.25) / 0.25, f(-0.5 - f(-0.51)) / 0.25] if prev_is_last else [0.0, f(f(0.1) - 0.25) / 0.25, f(-0.25 - f(-0.51)) / 0.25]
        want_v = [0.0, (0.0 - 0.25) / 0.25, f(f(-0.2) - f(-0.1)) / 0.25] if prev_is_last else [0.0, (0.0 - 0.25) / 0.25, f(0.25 - f(-0.1)) / 0.25]
        assert out["u_init_vel"].tolist() == want_u and out["v_init_vel"].tolist() == want_v
        assert (init == -1).all() and ts["init"][1, 0] == 75                     # reset in the copy, the (-1, 20) point included


def test_frame_reference_reproduces_the_oracles_frame_loop():
    """lvo.Frontend on the edge test's texture; for every steady-state frame the tracks and new points the oracle held before it go through
    track_ref (old and new), commit_ref (mode 0, then 1) and msg_ref on pyramids rebuilt from the same images: ids, points, lifetimes,
    descriptors, the LK counters and the message must be the oracle's"""
    from tests.test_gpu_frontend_edge import _texture, _crops, _walk, _imu, _cfg
    w, h = 320, 240
    cfg = _cfg(w, h, max_features_num=120, min_distance=12, pyramid_levels=3)
    frames = _crops(_texture(1, h + 120, w + 160), w, h, _walk(9))
    ora = lvo.Frontend(cfg)
    cam = (cfg["distortion_model"], cfg["intrinsics"], cfg["distortion"])
    ts_all = [1.0 + 0.05 * i for i in range(len(frames))]
    imu_all = _imu(ts_all[-1])
    pyr = lambda img: lvo.LkPyramid(lvo.clahe(img), cfg["patch_size"], cfg["pyramid_levels"])
    last_pub, checked, msgs, next_id = None, 0, 0, None
    for i, (ts, img) in enumerate(zip(ts_all, frames)):
        imu = imu_all[(imu_all["t"] < ts + 0.05)][-60:]
        before, new_before, state_before, stats_before = ora.tracks(), ora.new_pts(), ora.state, ora.lk_stats()
        have, msg = ora.process(img, ts, imu)
        if state_before == 1:
            last_pub = ts
        if state_before == 3 and len(before["ids"]) > 0:
            p0, p1 = pyr(frames[i - 1]), pyr(img)
            e0, e1 = p0.orb_prepare(), p1.orb_prepare()
            H = lvo.predict_homography(imu, ts_all[i - 1], ts, cfg["R_cam_imu"], cfg["intrinsics"])
            n0, n1, cap = len(before["ids"]), len(new_before), cfg["max_features_num"]
            if next_id is None:
                next_id = int(before["ids"].max()) + 1                         # the bootstrap numbered its survivors 0, 1, ...; from here on the reference counts
            t_old = R.track_ref(p0, p1, e0, e1, before["pts"], 0, before["desc"], H, cam, w, h)
            t_new = R.track_ref(p0, p1, e0, e1, new_before, 1, None, H, cam, w, h)
            src = dict(pts=before["pts"], curr=t_old["curr"], status=t_old["status"], und=t_old["und"], desc=before["desc"], id=before["ids"],
                       init=before["init"], life=before["lifetime"])
            d, st, br0 = R.commit_ref(0, cap, src, _dst(cap), dict(next_id=next_id, dst_n=0, n_new=n1, boot_ok=1))
            if n1:
                src = dict(pts=new_before, curr=t_new["curr"], status=t_new["status"], und=t_new["und"], desc=t_new["desc"])
                d, st, br1 = R.commit_ref(1, cap, src, d, st)
            after = ora.tracks()
            next_id = st["next_id"]
            n = st["dst_n"]
            assert n == len(after["ids"]) and n > 30
            assert np.array_equal(d["id"][:n], after["ids"]) and np.array_equal(d["life"][:n], after["lifetime"]) and np.array_equal(d["desc"][:n], after["desc"])
            assert np.array_equal(d["pts"][:n].view(np.uint32), after["pts"].view(np.uint32))
            a, b = ora.lk_stats(), stats_before
            assert (a[0] - b[0], a[1] - b[1]) == (t_old["point_levels"] + t_new["point_levels"], t_old["iterations"] + t_new["iterations"])
            if have:
                prev_is_last = ts_all[i - 1] == last_pub
                dt_1 = ts - ts_all[i - 1]
                out, init, _ = R.msg_ref(d, cap, n, cam, dt_1, dt_1 if prev_is_last else ts_all[i - 1] - last_pub, int(prev_is_last), K.MSG_STATE)
                assert out[:n].tobytes() == msg.tobytes()
                assert np.array_equal(init[:n].view(np.uint32), after["init"].view(np.uint32))
                msgs += 1
            else:
                assert np.array_equal(d["init"][:n].view(np.uint32), after["init"].view(np.uint32))
            checked += 1
        if have:
            last_pub = ts
    assert checked >= 4 and msgs >= 2


# ---- the reference half of every GPU case: the builder plus *_ref, held to the branch the case was built for
@pytest.mark.parametrize("name", list(K.TRACK_CASES))
def test_track_case_is_what_it_was_built_for(name):
    print(name, "alive / fwd / rev / orb:", K.check_track_case(K.track_case(name)))


def test_some_track_case_has_every_status_code():
    assert sum(1 for c in K.TRACK_CASES.values() if c[-1]) >= 2


@pytest.mark.parametrize("name", list(K.COMMIT_CASES))
def test_commit_case_is_what_it_was_built_for(name):
    K.check_commit_case(K.commit_case(name))


def test_commit_table_covers_what_it_must():
    cs = K.COMMIT_CASES.values()
    for wide, nt, caps in ((False, 256, (64, 512)), (True, 512, (513, 2048))):
        ns = {c["n"] for c in cs if c["mode"] == 0 and (c["cap"] > R.FM_WIDE_FROM) == wide}
        want = {0, 1, 63, 64, 65, nt - 1, nt, nt + 1, *caps} | ({2 * nt + 1} if wide else {2 * nt})      # 256 threads: no cap holds 2 NT + 1 points
        assert want <= ns, (nt, want - ns)
    for pat in ("all", "none", "third", "lane63", "last_chunk", "random4"):
        assert {(c["cap"] > 512) for c in cs if c["pattern"] == pat} == {False, True}, pat


@pytest.mark.parametrize("name", list(K.MSG_CASES))
def test_msg_case_is_what_it_was_built_for(name):
    K.check_msg_case(K.msg_case(name))
