"""The oracle's whole loop against the REFERENCE'S WHOLE PROGRAM: /root/reference/app/larvioMain.cpp with every src/*.cpp of the
reference, compiled where they lie (oracle/Makefile, target `ref` -> oracle/_ref/larvio_ref_full) - main(), the dataset readers, the
ImageProcessor, the LarVio filter with its static AND moving-start initialisers, linked into one executable that reads an ASL
directory and a configuration file like the shipped binary does.  Not the reference's: OpenCV's image algorithms (served by the
oracle's restatements, oracle/ref_shim3/ - for those this run says nothing new), cv::imread (the PNG reader of examples/), Eigen /
Ceres / boost (the stand-ins of oracle/ref_shim2/, ref_shim4/), and a headless pangolin that logs the pose main() hands to the viewer
after every odometry update (oracle/ref_shim5/pangolin/pangolin.h).  What this adds to the per-class pins: the two classes as main()
wires them - one IMU buffer shared by both (the filter erases, the front-end only reads), the 0.05 s look-ahead on the reader's
stamps, features handed over by pointer - on files, from image bytes to poses."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import lvo, lvo_be
from tests.test_gpu_zzz_ref_main import write_sequence, write_headline_sequence, write_workload_sequence
from tests.test_oracle_dynamic_init import replay  # noqa: F401  (the harness fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = os.path.join(ROOT, "oracle", "_ref", "larvio_ref_full")


def run_binary(binary, args, d, name):
    poses = os.path.join(d, name)
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=600, env=dict(os.environ, LVREF_MAIN_POSES=poses))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Totally" in r.stdout
    return np.loadtxt(poses, ndmin=2), r.stdout


def oracle_loop(args, fcfg, bcfg, frames):
    """larvioMain.cpp:84-117 with the oracle's two classes, on the stamps the reference's readers deliver (1e-9 * integer ns)"""
    t_img = [1e-9 * int(l.split(",")[0]) for l in open(args[1]).read().splitlines()[1:] if l.strip()]
    raw = np.loadtxt(args[0], delimiter=",", skiprows=1)
    imu = np.zeros(len(raw), lvo.IMU)
    imu["t"] = 1e-9 * raw[:, 0]; imu["gyro"] = raw[:, 1:4]; imu["acc"] = raw[:, 4:7]
    bcfg = dict(bcfg); grid = bcfg.pop("reference_grid_override", 1)
    fe = lvo.Frontend(fcfg); be = lvo_be.Ekf(dict(bcfg, reference_grid=grid))
    lo = 0; rows = []
    for t, (_, img) in zip(t_img, frames):
        hi = int(np.count_nonzero(imu["t"] - float(t) < 0.05))
        have, m = fe.process(img, float(t), imu[lo:hi])
        if have:
            upd, used = be.process(float(t), m, imu[lo:hi]); lo += used
            if upd:
                s = be.state(); rows.append(np.concatenate([s["p"], s["q"]]))
    return np.array(rows)


def test_the_references_whole_program_against_the_oracles_loop():
    if not os.path.exists(FULL):
        pytest.skip("oracle/_ref/larvio_ref_full not built (needs /root/reference: make -C oracle ref)")
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import TUMVI_LIKE
    from scipy.spatial.transform import Rotation
    d = tempfile.mkdtemp(prefix="lv", dir="/tmp")
    try:
        args = write_sequence(d, 64)
        M, out = run_binary(FULL, args, d, "poses_full.txt")
        cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
        fcfg = S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
        bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
        orc = oracle_loop(args, fcfg, bcfg, synth_frames(0, 64, cam=cam))
        assert len(orc) >= 15 and len(M) == len(orc), (len(M), len(orc))
        dp = np.abs(M[:, 12:15] - orc[:, :3]).max()
        # getTbw (larvio.cpp:2644-2658): linear() = R_b_w^T ... compared as rotations: the viewer's columns against the oracle's quaternion
        R_view = M[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(-1, 3, 3).transpose(0, 2, 1)       # column-major 4 x 4 -> R
        R_orc = Rotation.from_quat(orc[:, 3:7]).as_matrix()
        dR = min(np.abs(R_view - R_orc).max(), np.abs(R_view - R_orc.transpose(0, 2, 1)).max())
        print("the reference's whole program against the oracle's loop: %d poses, position %.2e m, rotation %.2e (%.2f m from the start)" % (len(M), dp, dR, np.linalg.norm(orc[-1, :3])))
        assert dp < 1e-6 and dR < 1e-6 and np.linalg.norm(orc[-1, :3]) > 0.3
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_moving_start_on_tracker_messages_product_host_code_against_the_references_initialiser(replay, tmp_path):
    """the start tests/test_gpu_zzz_ref_main.py's moving-start case goes through, rehearsed on the CPU: the messages the front-end publishes on
    frames 70.. of the synthetic sequence (the oracle's ImageProcessor = the reference's, byte for byte) handed to the reference's own
    DynamicInitializer (compiled in place) and to the PRODUCT's initialiser code (larvio_amd/csrc/be_init.h through the replay harness,
    cv::findFundamentalMat = the RANSAC restatement on both sides).  Asked: success on the same message with the same erase count, and
    the state the filter is started from to the minimisers' tolerance."""
    from oracle import lvref
    if not lvref.dyninit_available():
        pytest.skip("oracle/_ref/liblvref_dyninit.so not built")
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import TUMVI_LIKE
    from tests.test_oracle_dynamic_init import _record, _ang
    from scipy.spatial.transform import Rotation
    import json
    cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
    frames = synth_frames(70, 40, cam=cam)
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fe = lvo.Frontend(S.frontend_config(cam=cam, max_features_num=300, min_distance=15))
    msgs = []
    for t, img in frames:
        have, m = fe.process(img, t, imu[:int(np.count_nonzero(imu["t"] - t < 0.05))][-60:])
        if have:
            msgs.append((t, m))
    T = np.asarray(cam["T_cam_imu"], float); R_b2c = T[:3, :3]; t_c_b = -R_b2c.T @ T[:3, 3]
    Rf = lvref.dynamic_init(msgs, imu, R_b2c, t_c_b)
    assert Rf is not None
    rec = str(tmp_path / "start.txt"); _record(rec, dict(imu=imu, msgs=msgs), R_b2c, t_c_b)
    lvo.lib()
    P = json.loads(subprocess.run([replay, rec, os.path.join(ROOT, "oracle", "liblvo.so")], capture_output=True, text=True, check=True, timeout=300).stdout)
    d = dict(attitude=_ang(Rotation.from_quat(Rf["q"]).as_matrix(), Rotation.from_quat(P["q"]).as_matrix()),
             v=float(np.abs(Rf["v"] - np.array(P["v"])).max()), bg=float(np.abs(Rf["bg"] - np.array(P["bg"])).max()))
    print("tracker-made moving start: first success at message", Rf["message"], "| reference vs product host code", {k: "%.1e" % x for k, x in d.items()})
    assert Rf["message"] == P["message"] and Rf["state_time"] == P["state_time"] and Rf["erase"] == P["erase"]
    assert d["attitude"] < 1e-4 and d["v"] < 2e-3 and d["bg"] < 1e-5, d


def oracle_loop_from_motion(args, fcfg, bcfg, frames, initialiser, replay_of=None):
    """larvioMain.cpp:84-117 + LarVio::processFeatures:375-391 with the oracle's classes when nothing is handed in and the platform moves:
    every message goes to the moving-start initialiser (it sees the whole IMU buffer: nothing is erased before it succeeds); on success the
    filter starts from its state with the last ZUPT set to the state time (in-state features wait 5 s, larvio.cpp:384 / :1974), the
    initialiser's erase count applied, and the SAME message runs through propagation, observation, augmentation and update.
    replay_of = the record of an earlier run: the front-end is not run again (its messages depend on the filter only through the erase
    counts, which are asserted equal), only the initialiser - once, on the messages up to the recorded start - and the filter"""
    t_img = [1e-9 * int(l.split(",")[0]) for l in open(args[1]).read().splitlines()[1:] if l.strip()]
    raw = np.loadtxt(args[0], delimiter=",", skiprows=1)
    imu = np.zeros(len(raw), lvo.IMU); imu["t"] = 1e-9 * raw[:, 0]; imu["gyro"] = raw[:, 1:4]; imu["acc"] = raw[:, 4:7]
    T = np.asarray(bcfg["T_cam_imu"], float).reshape(4, 4); R_b2c = T[:3, :3]; t_c_b = -R_b2c.T @ T[:3, 3]
    be = lvo_be.Ekf(dict(bcfg, reference_grid=1))
    rows = []; record = []

    def start(st):
        be.set_state(st["state_time"], st["q"], np.zeros(3), st["v"], st["bg"], np.zeros(3), st["last_gyro"], st["last_acc"])
        be.set_last_zupt_time(st["state_time"])
        return int(st["erase"])
    if replay_of is not None:
        pre = [(t, m) for t, m, hi, used in replay_of if used is None]
        k = len(pre); t0, m0, hi0, _ = replay_of[k]
        started = initialiser(pre + [(t0, m0)], imu[:hi0], R_b2c, t_c_b)
        assert started is not None and started["message"] == k
        lo = start(started)
        for t, m, hi, used_before in replay_of[k:]:
            upd, used = be.process(t, m, imu[lo:hi]); lo += used
            assert used == used_before
            if upd:
                rows.append(be.state()["p"].copy())
        return np.array(rows), started, be.counters(), None
    fe = lvo.Frontend(fcfg); lo = 0; msgs = []; started = None
    for t, (_, img) in zip(t_img, frames):
        hi = int(np.count_nonzero(imu["t"] - float(t) < 0.05))
        have, m = fe.process(img, float(t), imu[lo:hi])
        if not have:
            continue
        if started is None:
            msgs.append((float(t), m))
            started = initialiser(msgs, imu[:hi], R_b2c, t_c_b)
            if started is None:
                record.append((float(t), m, hi, None))
                continue
            assert started["message"] == len(msgs) - 1
            lo = start(started)
        upd, used = be.process(float(t), m, imu[lo:hi]); lo += used
        record.append((float(t), m, hi, used))
        if upd:
            rows.append(be.state()["p"].copy())
    return np.array(rows), started, be.counters(), record


def test_moving_start_the_references_whole_program_against_the_oracles_loop():
    """the same, from a start in motion: nothing handed in, the reference's program has to come through its DynamicInitializer ("Dynamic
    initialization success !") and then runs 3.4 s of updates.  Against it: the oracle's front-end and filter with (a) the reference's own
    initialiser compiled in place - which leaves the filter's flow after a moving start as the only thing compared (2e-10 m measured; 3e-10 at the
    300-track budget of tests/test_gpu_zzz_ref_main.py's case) - and (b) the oracle's initialiser oracle/dyn_init.py, scipy's minimisers against the
    stand-in Ceres / solvePnP (measured 2e-6 m at 300 tracks)."""
    from oracle import lvref, dyn_init as D
    if not (os.path.exists(FULL) and lvref.dyninit_available()):
        pytest.skip("oracle/_ref not built (needs /root/reference: make -C oracle ref)")
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import TUMVI_LIKE
    d = tempfile.mkdtemp(prefix="lv", dir="/tmp")
    try:
        args = write_sequence(d, 90, first=70, max_features_num=120)       # (120 tracks: the oracle's bundle adjustment is scipy's lmdif)
        M, out = run_binary(FULL, args, d, "poses_full.txt")
        assert "Dynamic initialization success" in out and len(M) >= 20
        cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
        fcfg = S.frontend_config(cam=cam, max_features_num=120, min_distance=15)
        bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
        frames = synth_frames(70, 90, cam=cam)
        a, sa, ca, rec = oracle_loop_from_motion(args, fcfg, bcfg, frames, lvref.dynamic_init)
        b, sb, cb, _ = oracle_loop_from_motion(args, fcfg, bcfg, frames, lambda m, i, R, t: D.dynamic_init(m, i, R, t, fundamental=lambda p, q, th, cf: lvo.find_fundamental(p, q, th, cf)), replay_of=rec)
        assert len(a) == len(b) == len(M) and sa["message"] == sb["message"] and sa["erase"] == sb["erase"]
        da, db = np.abs(M[:, 12:15] - a).max(), np.abs(M[:, 12:15] - b).max()
        path = float(np.linalg.norm(np.diff(M[:, 12:15], axis=0), axis=1).sum())
        print("moving start, the reference's whole program against the oracle's loop: %d poses after message %d; with the reference's initialiser %.2e m, with the oracle's %.2e m (%.2f m travelled; %s)"
              % (len(M), sa["message"], da, db, path, ca))
        assert da < 1e-7 and db < 1e-4 and path > 0.1
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_headline_shape_with_in_state_features_the_references_whole_program_against_the_oracles_loop():
    """11.5 s of the headline shape (752 x 480 radtan, 150 tracks, 20-clone window) from rest, through the reference's whole program: static
    initialiser, four ZUPTs, take-off, and - 5 s after the last ZUPT (larvio.cpp:1974) - features entering the state (21 at the end,
    re-anchored at every pruning).  The oracle's loop with the reference's bookkeeping of features beyond the image bounds
    (reference_grid = 1, PARITY.md section 2) stays within 1e-8 m of it (4e-10 measured); with the older bookkeeping - the PRODUCT'S
    DEFAULT at the end of round 5 - the two part when the first border feature meets a full phantom cell (pose 87 of 105) and are 7 mm
    apart by the end: measured here so that the size of that known deviation is on record."""
    if not os.path.exists(FULL):
        pytest.skip("oracle/_ref/larvio_ref_full not built (needs /root/reference: make -C oracle ref)")
    d = tempfile.mkdtemp(prefix="lv", dir="/tmp")
    try:
        args, fcfg, bcfg, frames = write_headline_sequence(d, 230)
        M, out = run_binary(FULL, args, d, "poses_full.txt")
        res = {}
        for g in (1, 0):
            orc = oracle_loop(args, fcfg, dict(bcfg, reference_grid_override=g), frames)
            assert len(orc) == len(M) >= 90
            dd = np.linalg.norm(M[:, 12:15] - orc[:, :3], axis=1)
            res[g] = (float(dd.max()), int(np.argmax(dd > 1e-6)) if (dd > 1e-6).any() else None)
        print("headline shape, 230 frames, %d poses: the reference's whole program against the oracle's loop: reference_grid 1: %.2e m; 0: %.2e m, apart from pose %s on"
              % (len(M), res[1][0], res[0][0], res[0][1]))
        assert res[1][0] < 1e-8 and res[1][1] is None
        assert 1e-4 < res[0][0] < 5e-2          # the known deviation of the older bookkeeping, of this size
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_fisheye_shape_sw30_the_references_whole_program_against_the_oracles_loop():
    """configs[3]'s shape at the benchmarked window (512 x 512 equidistant, budget 300, sw_size 30, ZUPT on), 20 s from rest: 39 % of the
    observations have grid codes beyond the image bounds.  The oracle's loop (default = the reference's grid_map bookkeeping) within
    1e-8 m of the reference's whole program (2.9e-10 measured; the pre-round-6 bookkeeping: 3.2 cm, apart from pose 94 of 190 on).
    The same files go through the reference's main() on the product in tests/test_gpu_zzz_ref_main.py."""
    if not os.path.exists(FULL):
        pytest.skip("oracle/_ref/larvio_ref_full not built (needs /root/reference: make -C oracle ref)")
    d = tempfile.mkdtemp(prefix="lv", dir="/tmp")
    try:
        args, wl, frames = write_workload_sequence(d, "4", 400, max_features=300)
        M, out = run_binary(FULL, args, d, "poses_full.txt")
        orc = oracle_loop(args, wl["fcfg"], wl["bcfg"], frames)
        assert len(orc) == len(M) >= 180
        dd = np.linalg.norm(M[:, 12:15] - orc[:, :3], axis=1)
        print("configs[3] shape, sw_size 30, 400 frames, %d poses: the reference's whole program against the oracle's loop: %.2e m" % (len(M), dd.max()))
        assert dd.max() < 1e-8
    finally:
        shutil.rmtree(d, ignore_errors=True)


def test_the_shipped_configuration_file_end_to_end():
    """config/euroc.yaml as the reference ships it (the unchanged copy in tests/golden/ref_config/; only output_dir is pointed at a
    directory that exists): the reference's whole program reads it with its own loadParameters, the oracle's loop is configured by the
    product's loader (larvio_amd/config.py, the twin of include/lvk_config.hpp - held equal field by field in tests/test_oracle_ref_config.py)."""
    import re
    cfg_src = os.path.join(ROOT, "tests", "golden", "ref_config", "euroc.yaml")
    if not os.path.exists(FULL):
        pytest.skip("oracle/_ref/larvio_ref_full not built (make -C oracle ref)")
    from larvio_amd.config import load_config
    d = tempfile.mkdtemp(prefix="lv", dir="/tmp")
    try:
        args, _, _, frames = write_headline_sequence(d, 140)
        open(args[3], "w").write(re.sub(r'output_dir:\s*"[^"]*"', 'output_dir: "%s/logs/"' % d, open(cfg_src).read()))
        fcfg, bcfg = load_config(args[3])[:2]
        M, out = run_binary(FULL, args, d, "poses_full.txt")
        orc = oracle_loop(args, fcfg, bcfg, frames)
        assert len(M) == len(orc) >= 40
        dp = np.abs(M[:, 12:15] - orc[:, :3]).max()
        print("config/euroc.yaml end to end: %d poses, position %.2e m" % (len(M), dp))
        assert dp < 1e-8
    finally:
        shutil.rmtree(d, ignore_errors=True)
