"""GPU: lvk_vio_localise_map (VioDriver.localise_map) on the synthetic stream of tests/test_gpu_vio_driver.py.  The filter is started from the
ground truth at the second frame and run until it holds a clone for the frame just processed; the map is staged as
tests/test_gpu_frontend_reloc.py::staged_map does it - that frame's own corners (tests/orb_match_ref.frame_candidates) lifted to random
depths through the camera pose the call itself reports, taken into a yawed and shifted map frame, three bits of every descriptor inverted, a
quarter of the descriptors swapped among themselves, random distractors behind them.

same bits      the call equals the chain built by hand - ops.camera_pose_cov, match_map, ops.map_gather_obs, add_landmark_obs - in the
               landmark report, the state and the whole covariance after the next update, as bytes (two identical sessions side by side)
end to end     with the 99.9 % gate the batch is APPLIED and uses at least the true members a hand check finds (HAND_COUNT below)
nothing seen   a map behind the camera: an empty batch, ALL_REJECTED, and a ten-frame run with a call behind every frame keeps its bits
no clone       before initialisation, or a time between two clones: LVK_LOCALISE_NO_CLONE, nothing queued
refusals       no map, between begin and process (an undrained pipe), a shard transport; the handles go on"""
import numpy as np
import pytest

from tests import align_cases as AC
from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu

PSI, SHIFT = 0.7, np.array([4.0, -3.0, 0.8])
UNIT = (1.0, 1.0, 0.0, 0.0)
SIGMA_PX = 1.0
GATE_999 = 134.7
# True members of the staged map that the hand check finds inside their search radius with an unswapped descriptor: 432 of 575 with
# seed 5 (measured on an MI355X; the batch then carried 437 observations and used all of them).  The seed must give at least 20.
HAND_COUNT_MIN = 20


def _R2q(Rm):
    from larvio_amd import synthetic as S
    return S.R2q(Rm)


@pytest.fixture(scope="module")
def stream():
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    frames = synth_frames(40, 70)[:40]
    seq = S.imu_only_sequence()
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    return frames, seq, imu_all, S.frontend_config(max_features_num=150), S.backend_config(sw_size=15, if_zupt_valid=0)


class Session:
    """front-end + filter + VioDriver on one context, started from the ground truth at frame 1"""

    def __init__(self, ctx, stream, pipe_ctx=None):
        import larvio_amd
        from larvio_amd.vio import VioDriver, VioPipeline
        self.frames, self.seq, self.imu, fcfg, bcfg = stream
        self.fcfg = fcfg
        self.fe = larvio_amd.ImageProcessor(fcfg, ctx); assert self.fe.initialize()
        self.be = larvio_amd.LarVio(bcfg, pipe_ctx or ctx); assert self.be.initialize()
        self.drv = (VioPipeline if pipe_ctx else VioDriver)(self.fe, self.be, self.imu)
        self.pipe = pipe_ctx is not None
        self.i = 0

    def step(self):
        """one frame -> (has_msg, updated)"""
        t, img = self.frames[self.i]
        if self.i == 1:
            if self.pipe:
                self.drv.drain()
            k = int(np.searchsorted(self.imu["t"], t, side="right")) - 1
            t0 = self.imu["t"][k]; tr = self.seq.traj
            self.be.set_state(t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), self.imu["gyro"][k], self.imu["acc"][k])
        r = self.drv.step(t, self.drv.visible_end(t), img=img)
        self.i += 1
        return (r, r) if self.pipe else r

    def run_to_clone(self, at_least=10):
        """until a frame at or behind `at_least` has published and updated: the filter then holds a clone for the frame just processed"""
        while True:
            has, upd = self.step()
            if self.i > at_least and has and upd:
                return self.frames[self.i - 1]

    def next_update(self):
        while True:
            has, upd = self.step()
            if has and upd:
                return

    def snapshot(self):
        st = self.be.state()
        return b"".join(np.ascontiguousarray(st[k]).tobytes() for k in sorted(st)) + self.be.cov().tobytes() + self.be.clones().tobytes()

    def close(self):
        if self.pipe:
            self.drv.close()
        self.be.close(); self.fe.close()


def stage_map(fcfg, pts, desc, R_wc, p_wc, n_total, seed):
    """test_gpu_frontend_reloc.staged_map with the pose given -> (X, cov, descriptors, is_swapped)"""
    from oracle import lvo
    rng = np.random.default_rng(seed)
    n = len(pts)
    und = lvo.undistort(pts, fcfg["intrinsics"], fcfg["distortion_model"], fcfg["distortion"], UNIT).astype(np.float64)
    z = rng.uniform(2.0, 9.0, n)
    p_w = np.column_stack([und * z[:, None], z]) @ R_wc.T + p_wc
    X_true = (p_w - SHIFT) @ AC.rz(PSI)                                            # p_w = Rz X + shift
    d_true = desc.copy(); d_true[:, 0] ^= 0x15
    swapped = rng.permutation(n)[:n // 4]
    d_true[swapped] = d_true[np.roll(swapped, 1)]
    is_swapped = np.zeros(n, bool); is_swapped[swapped] = True
    m = n_total - n
    X = np.concatenate([X_true, rng.uniform(-30.0, 30.0, (m, 3))])
    d = np.concatenate([d_true, rng.integers(0, 256, (m, 32), dtype=np.uint8)])
    cov = np.tile(1e-4 * np.eye(3), (n_total, 1, 1))
    return X, cov, d, is_swapped


def behind_map(R_wc, p_wc, n=200, seed=3):
    """points 3 .. 12 m behind the camera, with random descriptors"""
    rng = np.random.default_rng(seed)
    pc = np.column_stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), -rng.uniform(3, 12, n)])
    return pc @ R_wc.T + p_wc, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def pose_of_last_clone(s):
    from larvio_amd import localize
    cl = s.be.clones(); st = s.be.state()
    return localize.camera_pose(cl[-1], (st["R_b2c"], st["t_c_b"]))


ALIGN = (np.cos(PSI), np.sin(PSI), SHIFT)


@pytest.fixture(scope="module")
def staged(gpu_ctx, stream):
    """one session run to its clone, a probe call on a map behind the camera for the pose the call reports, and the map staged through
    that pose - computed once, shared by the tests below"""
    from larvio_amd._lib import LOCALISE_QUEUED
    s = Session(gpu_ctx, stream)
    t, img = s.run_to_clone()
    R0, p0 = pose_of_last_clone(s)
    Xb, db = behind_map(R0, p0)
    s.fe.set_map(Xb, None, db)
    cid = int(s.be.clones()["id"][-1])
    info = s.drv.localise_map(clone_id=cid, sigma_px=SIGMA_PX)
    assert info["status"] == LOCALISE_QUEUED and info["clone_id"] == cid
    assert np.array_equal(info["R_wc"], R0) and np.array_equal(info["p_wc"], p0)       # localize.camera_pose is the call's pose, bit for bit
    pts, desc = R.frame_candidates(stream[3], img)
    X, cov, d, sw = stage_map(stream[3], pts, desc, info["R_wc"].copy(), info["p_wc"].copy(), len(pts) + 1500, seed=5)
    s.close()
    return dict(pts=pts, desc=desc, X=X, cov=cov, d=d, swapped=sw, Xb=Xb, db=db, R_wc=info["R_wc"].copy(), p_wc=info["p_wc"].copy(), frame=s.i - 1)


def test_call_is_the_chain_built_by_hand(gpu_ctx, stream, staged):
    """two identical sessions; one calls lvk_vio_localise_map, the other builds the batch by hand through the stage entries; after the
    next update the landmark report, the state and the whole covariance agree as bytes.  (Cannot pass without the call.)"""
    from larvio_amd import ops
    from larvio_amd._lib import LOCALISE_QUEUED, MATCH_OK
    sel = ops.map_select_options()
    out = []
    for mode in ("call", "hand"):
        s = Session(gpu_ctx, stream)
        s.run_to_clone()
        assert s.i - 1 == staged["frame"]
        s.fe.set_map(staged["X"], staged["cov"], staged["d"])
        s.be.set_landmark_options(GATE_999, 0.1)
        cl = s.be.clones(); cid = int(cl["id"][-1]); st = s.be.state()
        if mode == "call":
            info = s.drv.localise_map(align=ALIGN, clone_id=cid, sigma_px=SIGMA_PX, select=sel, tag=7)
            assert info["status"] == LOCALISE_QUEUED and info["n_bad"] == 0
            n_ok = int(info["n_ok"]); pose = (info["R_wc"].copy(), info["p_wc"].copy(), info["cov_cam"].copy()); minfo = info["map"].copy()
        else:
            P = s.be.cov()
            leg = s.be.dim - 6 * len(cl) - len(s.be.features()[0])
            job = ops.camera_pose_job(leg + 6 * (len(cl) - 1), cl["q"][-1], cl["p"][-1], st["R_b2c"], st["t_c_b"])
            R_wc, p_wc, cov_cam = ops.camera_pose_cov(s.be.ctx, P, job)
            rec, minfo = s.fe.match_map(R_wc, p_wc, align=ALIGN, cov_cam=cov_cam, select=sel)
            fx, fy = s.fcfg["intrinsics"][:2]
            g = ops.map_gather_obs(gpu_ctx, rec, staged["X"], staged["cov"], SIGMA_PX / ((fx + fy) / 2), align=ALIGN)
            assert int(g["info"]["n_bad"]) == 0
            n_ok = len(g["obs"]); pose = (R_wc, p_wc, cov_cam)
            assert n_ok == int((rec["m"]["status"] == MATCH_OK).sum())
            s.be.add_landmark_obs(g["obs"]["p_w"], g["obs"]["uv"], g["obs"]["sigma"], g["obs"]["cov_w"], clone_id=cid, tag=7)
        s.next_update()
        rep = s.be.take_landmark_reports()
        out.append(dict(n_ok=n_ok, pose=pose, minfo=minfo, rep=rep, snap=s.snapshot(), stats=s.be.landmark_stats()))
        s.close()
    a, b = out
    assert a["n_ok"] == b["n_ok"] and a["n_ok"] >= HAND_COUNT_MIN
    assert all(np.array_equal(x, y) for x, y in zip(a["pose"], b["pose"]))
    assert a["minfo"].tobytes() == b["minfo"].tobytes()
    assert len(a["rep"]) == 1 and a["rep"].tobytes() == b["rep"].tobytes(), (a["rep"], b["rep"])
    assert a["stats"] == b["stats"]
    assert a["snap"] == b["snap"]


def test_end_to_end_applied(gpu_ctx, stream, staged):
    """the 99.9 % gate: APPLIED, and n_used is at least the true members a hand check finds inside the search radius with an unswapped
    descriptor.  Measured with seed 5: see HAND_COUNT_MIN and the printed count."""
    from larvio_amd import localize, ops
    from larvio_amd._lib import LOCALISE_QUEUED
    from larvio_amd.larvio import LANDMARK_REPORT  # noqa: F401
    s = Session(gpu_ctx, stream)
    s.run_to_clone()
    s.fe.set_map(staged["X"], staged["cov"], staged["d"])
    s.be.set_landmark_options(GATE_999, 0.1)
    t_clone = float(s.be.clones()["time"][-1])
    before = s.snapshot()
    info = s.drv.localise_map(align=ALIGN, time=t_clone, sigma_px=SIGMA_PX, tag=11)           # the clone by its time
    assert info["status"] == LOCALISE_QUEUED and info["clone_id"] == int(s.be.clones()["id"][-1])
    assert s.snapshot() == before and s.be.landmark_stats()["waiting"] == 1               # queued, nothing applied yet
    # the hand check: project the true members through the reported pose; inside the smallest radius the selection can give (r_min = 4 px)
    n = len(staged["pts"])
    p_w, _ = localize.apply_alignment(dict(c=ALIGN[0], s=ALIGN[1], t=ALIGN[2]), staged["X"][:n])
    px, ok = localize.predict_pixels(p_w, info["R_wc"], info["p_wc"], s.fcfg)
    near = ok & (np.hypot(*(px - staged["pts"]).T) <= 4.0)
    hand = int((near & ~staged["swapped"]).sum())
    s.next_update()
    rep = s.be.take_landmark_reports()
    print(f"hand count {hand} of {n} true members; report {rep}")
    assert hand >= HAND_COUNT_MIN
    assert len(rep) == 1 and rep["tag"][0] == 11 and rep["status"][0] == 0 and rep["n_obs"][0] == info["n_ok"], rep      # LVK_LANDMARKS_APPLIED
    assert rep["n_used"][0] >= hand, (rep, hand)
    assert s.snapshot() != before
    s.close()


def test_nothing_visible_and_no_disturbance(gpu_ctx, stream, staged):
    """a map behind the camera: n_selected = 0, an empty batch, ALL_REJECTED; ten frames with a call behind every frame publish the bits
    of a run without (frames without a clone answer NO_CLONE and queue nothing)"""
    from larvio_amd._lib import LOCALISE_QUEUED, LOCALISE_NO_CLONE
    runs = []
    for call in (False, True):
        s = Session(gpu_ctx, stream)
        s.run_to_clone()
        s.fe.set_map(staged["Xb"], None, staged["db"])
        msgs = []; n_q = 0
        for _ in range(10):
            if call:
                cl = s.be.clones()
                info = s.drv.localise_map(clone_id=int(cl["id"][-1]), sigma_px=SIGMA_PX, tag=s.i)
                assert info["status"] == LOCALISE_QUEUED and info["map"]["n_selected"] == 0 and info["n_ok"] == 0 and info["map"]["n_behind"] == len(staged["Xb"])
                n_q += 1
                between = 0.5 * (cl["time"][-1] + cl["time"][-2])
                assert s.drv.localise_map(time=float(between), sigma_px=SIGMA_PX)["status"] == LOCALISE_NO_CLONE
            s.step()
            msgs.append(s.fe.tracks()["pts"].tobytes())
        s.next_update()
        if call:
            rep = s.be.take_landmark_reports()
            assert len(rep) == n_q and (rep["status"] == 1).all() and (rep["n_obs"] == 0).all(), rep          # LVK_LANDMARKS_ALL_REJECTED
            assert s.be.landmark_stats()["queued"] == n_q
        runs.append((msgs, s.snapshot()))
        s.close()
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]


def test_no_clone(gpu_ctx, stream, staged):
    from larvio_amd._lib import LOCALISE_NO_CLONE
    s = Session(gpu_ctx, stream)
    s.fe.set_map(staged["Xb"], None, staged["db"])
    s.step()                                                                               # one frame, the filter is not initialised
    q0 = s.be.landmark_stats()["queued"]
    for kw in (dict(clone_id=0), dict(time=s.frames[0][0])):
        info = s.drv.localise_map(sigma_px=SIGMA_PX, **kw)
        assert info["status"] == LOCALISE_NO_CLONE and info["clone_id"] == -1 and info["n_ok"] == 0 and not info["R_wc"].any()
    s.run_to_clone()
    cl = s.be.clones()
    for kw in (dict(time=float(0.5 * (cl["time"][-1] + cl["time"][-2]))), dict(clone_id=int(cl["id"][-1]) + 1000), dict(time=float(cl["time"][-1]) + 1.0)):
        assert s.drv.localise_map(sigma_px=SIGMA_PX, **kw)["status"] == LOCALISE_NO_CLONE
    assert s.be.landmark_stats()["queued"] == q0 and s.be.landmark_stats()["waiting"] == 0
    s.close()


def test_refusals(gpu_ctx, stream, staged):
    """each refusal raises, queues nothing, and the handles go on"""
    import ctypes as C
    import larvio_amd
    from larvio_amd import sharding
    from larvio_amd._lib import lib, make_image, LOCALISE_QUEUED
    s = Session(gpu_ctx, stream)
    s.run_to_clone()
    cid = lambda: int(s.be.clones()["id"][-1])
    with pytest.raises(larvio_amd.LvkError, match="no map is set"):
        s.drv.localise_map(clone_id=cid())
    s.fe.set_map(staged["Xb"], None, staged["db"])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(larvio_amd.LvkError, match="sigma_px"):
            s.drv.localise_map(clone_id=cid(), sigma_px=bad)
    with pytest.raises(larvio_amd.LvkError, match="clone_id"):
        s.drv.localise_map(clone_id=-2)
    # between lvk_frontend_begin and lvk_frontend_process of the same frame
    L = lib()
    t, img = s.frames[s.i]
    im, keep = make_image(img)
    L.lvk_frontend_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_double]; L.lvk_frontend_begin.restype = C.c_int
    assert L.lvk_frontend_begin(s.fe._h, C.byref(im), float(t)) == 0
    with pytest.raises(larvio_amd.LvkError, match="still waiting for its lvk_frontend_process"):
        s.drv.localise_map(clone_id=cid())
    s.step()                                                                               # the frame's own process call: the handle goes on
    # a shard transport
    cb = sharding.EXCHANGE_FN(lambda user, d_send, d_recv, nbytes, stream: 0)              # never called: the transport is cleared before the next update
    s.be.set_shard(0, 1, C.cast(cb, C.c_void_p), None, keepalive=cb)
    with pytest.raises(larvio_amd.LvkError, match="sharded"):
        s.drv.localise_map(clone_id=cid())
    s.be.set_shard(0, 1, None, None)
    assert s.be.landmark_stats()["queued"] == 0
    assert s.drv.localise_map(clone_id=cid())["status"] == LOCALISE_QUEUED                 # and both handles go on
    s.next_update()
    assert len(s.be.take_landmark_reports()) == 1
    s.close()


def test_undrained_pipe(gpu_ctx, stream, staged):
    """VioPipeline.localise_map raises between a step and the drain that follows, and works after drain()"""
    import larvio_amd
    from larvio_amd._lib import LOCALISE_QUEUED
    ctx2 = larvio_amd.Context(0)
    s = Session(gpu_ctx, stream, pipe_ctx=ctx2)
    for _ in range(12):
        s.step()
    with pytest.raises(ValueError, match="drain"):
        s.drv.localise_map(clone_id=0)
    s.drv.drain()
    s.fe.set_map(staged["Xb"], None, staged["db"])
    info = s.drv.localise_map(clone_id=int(s.be.clones()["id"][-1]))
    assert info["status"] == LOCALISE_QUEUED and info["map"]["n_selected"] == 0
    s.step(); s.step(); s.step()
    s.drv.drain()
    assert len(s.be.take_landmark_reports()) == 1
    s.close()
    ctx2.close()
