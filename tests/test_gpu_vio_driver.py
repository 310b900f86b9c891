"""GPU parity of the WHOLE hot path through the single driver-step entry point lvk_vio_process: frames in, filter state out,
with the driver's shared IMU buffer (app/larvioMain.cpp:87-117: visible up to t_img + 0.05, erased by processFeatures).
Front-end message identity is implied: any differing track id / coordinate would change the filter state beyond 1e-5."""
import numpy as np
import pytest

from tests.cov_compare import block_name, corr_error, CORR

pytestmark = pytest.mark.gpu
REL = 1e-5


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _R2q(R):
    t = np.trace(R); s = np.sqrt(t + 1) * 2
    return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])


@pytest.mark.parametrize("device_frames", [False, True])
def test_driver_loop_matches_oracle(gpu_ctx, device_frames):
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver
    from oracle import lvo, lvo_be
    from tests.conftest import synth_frames
    frames = synth_frames(40, 70)
    seq = S.imu_only_sequence()
    ts = [f[0] for f in frames]
    k_lo = max(int(ts[0] * 200) - 4, 0)
    imu_all = seq.imu_array(k_lo, int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(max_features_num=150)
    bcfg = S.backend_config(sw_size=15, if_zupt_valid=0)
    fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
    be = larvio_amd.LarVio(bcfg, gpu_ctx); assert be.initialize()
    ofe = lvo.Frontend(fcfg); obe = lvo_be.Ekf(bcfg)
    drv = VioDriver(fe, be, imu_all)
    d_frames = None
    if device_frames:
        d_frames = gpu_ctx.to_device(np.stack([f[1] for f in frames]))      # frames already in HBM (camera DMA case)
    lo = 0; n_upd = 0; worst = 0.0; worst_c, worst_c_at = 0.0, ""
    for i, (t, img) in enumerate(frames):
        hi = drv.visible_end(t)
        if i == 1:
            k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
            t0 = imu_all["t"][k]; tr = seq.traj
            a = (t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            obe.set_state(*a); be.set_state(*a)
        assert drv.lo == lo
        buf = imu_all[lo:hi]
        have_o, m = ofe.process(img, t, buf)
        upd_o = False
        if have_o:
            upd_o, used = obe.process(t, m, buf); lo += used
        if device_frames:
            has_g, upd_g = drv.step(t, hi, device_ptr=d_frames.ptr + i * img.size, stride=img.shape[1])
        else:
            has_g, upd_g = drv.step(t, hi, img=img)
        assert has_g == have_o and upd_g == bool(upd_o), (i, has_g, have_o, upd_g, upd_o)
        if not upd_o:
            continue
        n_upd += 1
        assert be.dim == obe.dim
        so, sg = obe.state(), be.state()
        for k in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"):
            e_k = _rel(sg[k], so[k])
            if e_k > worst:
                worst = e_k; _WORST_AT.update(update=n_upd, frame=i, what=k, detail="max|ref| %.3e, abs diff %.3e" % (np.abs(so[k]).max(), np.abs(np.asarray(sg[k]) - so[k]).max()))
        Pg, Po = be.cov(), obe.cov()
        e_p = _rel(Pg, Po)
        if e_p > worst:
            # which entry of P carries it: the block names of its row and column, its own size against the largest entry of P
            ij = np.unravel_index(np.argmax(np.abs(Pg - Po)), Po.shape); leg = 46 if bcfg.get("calib_imu_instrinsic") else 22
            nc = len(obe.clones()["id"])
            def blk(x):
                return block_name(x, leg, nc)
            worst = e_p; _WORST_AT.update(update=n_upd, frame=i, what="P", detail=f"entry ({blk(ij[0])},{blk(ij[1])}) = {Po[ij]:.3e} differs by {abs(Pg[ij] - Po[ij]):.3e}; max|P| = {np.abs(Po).max():.3e} "
                                          f"at {blk(np.unravel_index(np.argmax(np.abs(Po)), Po.shape)[0])}; rows of the last update {be.counters().get('last_rows')}")
        assert np.array_equal(be.clones()["id"], obe.clones()["id"])
        assert np.array_equal(be.features()[0], obe.features()[0])
        assert worst < REL, (i, worst)
        e_c, at = corr_error(Pg, Po, 46 if bcfg.get("calib_imu_instrinsic") else 22, len(obe.clones()["id"]))
        if e_c > worst_c:
            worst_c, worst_c_at = e_c, f"update {n_upd}, frame {i}: {at}"
        assert np.isfinite(e_c) and worst_c < CORR, (i, e_c, at, worst_c, worst_c_at)
    assert n_upd >= 25
    tg, to = fe.tracks(), ofe.tracks()
    assert np.array_equal(tg["ids"], to["ids"]) and np.array_equal(tg["pts"], to["pts"])
    co, cg = obe.counters(), be.counters()
    for k in ("hybrid", "msckf", "gated_in", "gated_out", "map"):
        assert cg[k] == co[k]
    print("driver loop parity: updates", n_upd, "worst rel", worst)
    print(f"correlation-scaled P error: worst {worst_c:.3e} ({worst_c_at or 'Pg == Po at every update'})")


def _disturb(frames):
    """a black frame, two frames of unrelated noise, a camera frozen for five frames"""
    frames = list(frames)
    h, w = frames[0][1].shape
    rng = np.random.default_rng(9)
    frames[22] = (frames[22][0], np.zeros((h, w), np.uint8))
    for k in (36, 37):
        frames[k] = (frames[k][0], rng.integers(0, 256, (h, w)).astype(np.uint8))
    for k in range(50, 55):
        frames[k] = (frames[k][0], frames[49][1])
    return frames


@pytest.mark.parametrize("disturbed", [False, True, "headline"])
def test_pipelined_driver_is_identical_to_sequential(gpu_ctx, disturbed):
    """lvk_vio_pipe_*: front-end of frame k+1 overlapping the update of frame k on a second stream gives the same bits as the
    sequential driver step (same library, same kernels — only the schedule differs), hence the same parity with the oracle."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver, VioPipeline
    from tests.conftest import synth_frames
    headline = disturbed == "headline"            # BASELINE.json's configuration: 150-feature budget, sw_size 30, window full and cycling
    frames = synth_frames(40, 140 if headline else 70)
    if disturbed is True:
        frames = _disturb(frames)
    seq = S.imu_only_sequence()
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(max_features_num=150)
    bcfg = (S.backend_config(sw_size=30, max_features=150) if headline else
            S.backend_config(sw_size=20, if_zupt_valid=1) if disturbed else S.backend_config(sw_size=15, if_zupt_valid=0))
    ctx2 = larvio_amd.Context(0)                                    # second context = second stream, for the filter
    out = []
    for mode in ("seq", "pipe"):
        fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(bcfg, ctx2 if mode == "pipe" else gpu_ctx); assert be.initialize()
        drv = (VioPipeline if mode == "pipe" else VioDriver)(fe, be, imu_all)
        n_msg = 0
        for i, (t, img) in enumerate(frames):
            if i == 1:
                if mode == "pipe":
                    drv.drain()
                k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
                t0 = imu_all["t"][k]; tr = seq.traj
                be.set_state(t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            r = drv.step(t, drv.visible_end(t), img=img)
            n_msg += int(r if mode == "pipe" else r[0])
        if mode == "pipe":
            n_upd, n_m = drv.drain()
            assert n_m == n_msg
            early, wrong = drv.early_counts()          # erase counts taken before the running update had finished: all confirmed
            assert wrong == 0, (early, wrong)
            print("pipelined driver: %d messages, %d erase counts taken early, %d wrong" % (n_m, early, wrong))
            drv.close()
        st = be.state()
        out.append((n_msg, be.dim, {k: np.array(v, copy=True) for k, v in st.items()}, be.cov(), be.clones()["id"].copy(), be.features()[0].copy(),
                    be.counters(), fe.tracks()))
        be.close(); fe.close()
    ctx2.close()
    a, b = out
    if headline:
        assert len(a[4]) >= 28 and a[6]["msckf"] >= 5, (len(a[4]), a[6])       # the 28 -> 30 cycle ran, with pruning MSCKF updates
    assert a[0] == b[0] and a[1] == b[1] and a[0] >= 30
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k
    assert np.array_equal(a[3], b[3])
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and a[6] == b[6]
    for k in ("ids", "pts", "lifetime"):
        assert np.array_equal(a[7][k], b[7][k])


def test_deferred_update_is_identical_to_blocking(gpu_ctx):
    """lvk_ekf_process_async / lvk_vio_process_deferred - what the adapter classes do under the reference's blocking drivers
    (processImage; processFeatures returns at once, the update runs on the filter's worker thread; getters wait): the headline
    configuration through 140 frames, (a) reading the pose right after every processFeatures as app/larvioMain.cpp:139 does and (b) one
    frame late, against the blocking driver step: every pose read, the final state, covariance, id lists, counters and tracks identical."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver, VioDeferred
    wl = S.workload("A")
    first = int(2.0 * wl["img_rate"]); n = 140
    from tests.conftest import synth_frames
    fr = synth_frames(first, n, cam=wl["cam"], img_rate=wl["img_rate"])
    seq = S.imu_only_sequence(cam=wl["cam"])
    imu_all = seq.imu_array(max(int(fr[0][0] * 200) - 4, 0), int(fr[-1][0] * 200) + 40)
    ctx2 = larvio_amd.Context(0)
    out = []
    for mode in ("blocking", "immediate", "late"):
        fe = larvio_amd.ImageProcessor(wl["fcfg"], gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(wl["bcfg"], gpu_ctx if mode == "blocking" else ctx2); assert be.initialize()
        drv = (VioDriver if mode == "blocking" else VioDeferred)(fe, be, imu_all)
        poses = []; owed = False
        for i, (t, img) in enumerate(fr):
            if i == 1:
                k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
                t0 = imu_all["t"][k]; tr = seq.traj
                be.set_state(t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            has, upd = drv.step(t, drv.visible_end(t), img=img)
            if mode == "late":
                if upd:
                    owed = True
                elif owed:                                # the frame after an update: its front-end ran while the update was in flight
                    be.state(); owed = False
            elif upd:
                st = be.state(); poses.append(np.concatenate([st["q"], st["p"], st["v"]]))
        if mode != "blocking":
            be.wait()                                     # raises if the last deferred update failed
        st = be.state()
        out.append((np.array(poses), {k: np.array(v, copy=True) for k, v in st.items()}, be.cov(), be.clones()["id"].copy(), be.features()[0].copy(), be.counters(), fe.tracks()))
        be.close(); fe.close()
    ctx2.close()
    a = out[0]
    assert len(a[0]) >= 65 and len(a[3]) >= 28 and a[5]["msckf"] >= 5
    for b in out[1:]:
        for k in a[1]:
            assert np.array_equal(a[1][k], b[1][k]), k
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5]
        for k in ("ids", "pts", "lifetime"):
            assert np.array_equal(a[6][k], b[6][k])
    assert np.array_equal(out[0][0], out[1][0])          # pose after EVERY update, read immediately: identical to the blocking call


def S_EUROC():
    from larvio_amd import synthetic as S
    return dict(S.EUROC)


TUMVI_LIKE = dict(
    width=512, height=512, intrinsics=(190.978, 190.973, 254.932, 256.897), distortion_model=1,      # equidistant (config 4 shape)
    distortion=(0.0034823894, 0.0007150348, -0.0020532361, 0.0002029367),
    T_cam_imu=None)


_WORST_AT = {}      # where the worst relative error of the last _driver_pair run sat (printed by the whole-loop tests)


def _driver_pair(gpu_ctx, cam, first, count, fcfg_over, bcfg_over, init_from_gt, min_updates, mutate=None, oracle_threads=1, workload=None):
    """oracle loop vs VioDriver on frames [first, first+count) of the synthetic sequence seen through `cam`
    (workload: a larvio_amd.synthetic.workload() dict - camera, frame rate and both configurations exactly as bench.py runs them)"""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver
    from oracle import lvo, lvo_be
    from tests.conftest import synth_frames
    img_rate = 20.0
    if workload is not None:
        cam, img_rate = workload["cam"], workload["img_rate"]
    cam = dict(cam)
    if cam.get("T_cam_imu") is None:
        cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
    frames = synth_frames(first, count, cam=cam, img_rate=img_rate)
    if mutate is not None:
        frames = mutate(list(frames))
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    if workload is not None:
        fcfg, bcfg = dict(workload["fcfg"], **fcfg_over), dict(workload["bcfg"], **bcfg_over)
    else:
        fcfg = S.frontend_config(cam=cam, **fcfg_over)
        bcfg = S.backend_config(cam=cam, **bcfg_over)
    fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
    be = larvio_amd.LarVio(bcfg, gpu_ctx); assert be.initialize()
    ofe = lvo.Frontend(fcfg); obe = lvo_be.Ekf(bcfg)
    lvo.set_threads(oracle_threads)                # same bits for any count (tests/test_oracle_frontend.py); only the wall time changes
    drv = VioDriver(fe, be, imu_all)
    lo = 0; n_upd = 0; worst = 0.0; worst_c, worst_c_at = 0.0, ""
    for i, (t, img) in enumerate(frames):
        hi = drv.visible_end(t)
        if init_from_gt and i == 1:
            k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
            t0 = imu_all["t"][k]; tr = seq.traj
            a = (t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            obe.set_state(*a); be.set_state(*a)
        buf = imu_all[lo:hi]
        have_o, m = ofe.process(img, t, buf)
        upd_o = False
        if have_o:
            upd_o, used = obe.process(t, m, buf); lo += used
        has_g, upd_g = drv.step(t, hi, img=img)
        assert has_g == have_o and upd_g == bool(upd_o) and drv.lo == lo, (i, has_g, have_o, upd_g, upd_o)
        if not upd_o:
            continue
        n_upd += 1
        assert be.dim == obe.dim
        so, sg = obe.state(), be.state()
        for k in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"):
            e_k = _rel(sg[k], so[k])
            if e_k > worst:
                worst = e_k; _WORST_AT.update(update=n_upd, frame=i, what=k, detail="max|ref| %.3e, abs diff %.3e" % (np.abs(so[k]).max(), np.abs(np.asarray(sg[k]) - so[k]).max()))
        Pg, Po = be.cov(), obe.cov()
        e_p = _rel(Pg, Po)
        if e_p > worst:
            # which entry of P carries it: the block names of its row and column, its own size against the largest entry of P
            ij = np.unravel_index(np.argmax(np.abs(Pg - Po)), Po.shape); leg = 46 if bcfg.get("calib_imu_instrinsic") else 22
            nc = len(obe.clones()["id"])
            def blk(x):
                return block_name(x, leg, nc)
            worst = e_p; _WORST_AT.update(update=n_upd, frame=i, what="P", detail=f"entry ({blk(ij[0])},{blk(ij[1])}) = {Po[ij]:.3e} differs by {abs(Pg[ij] - Po[ij]):.3e}; max|P| = {np.abs(Po).max():.3e} "
                                          f"at {blk(np.unravel_index(np.argmax(np.abs(Po)), Po.shape)[0])}; rows of the last update {be.counters().get('last_rows')}")
        assert np.array_equal(be.clones()["id"], obe.clones()["id"]) and np.array_equal(be.features()[0], obe.features()[0])
        assert worst < REL, (i, worst)
        e_c, at = corr_error(Pg, Po, 46 if bcfg.get("calib_imu_instrinsic") else 22, len(obe.clones()["id"]))
        if e_c > worst_c:
            worst_c, worst_c_at = e_c, f"update {n_upd}, frame {i}: {at}"
        assert np.isfinite(e_c) and worst_c < CORR, (i, e_c, at, worst_c, worst_c_at)
    assert n_upd >= min_updates
    print(f"correlation-scaled P error: worst {worst_c:.3e} ({worst_c_at or 'Pg == Po at every update'})")
    tg, to = fe.tracks(), ofe.tracks()
    assert np.array_equal(tg["ids"], to["ids"]) and np.array_equal(tg["pts"], to["pts"])
    co, cg = obe.counters(), be.counters()
    for k in ("hybrid", "msckf", "zupt", "gated_in", "gated_out", "map"):
        assert cg[k] == co[k], (k, cg, co)
    n_clones = len(obe.clones()["id"]); dim = obe.dim
    be.close(); fe.close()
    lvo.set_threads(1)
    if workload is not None:
        return n_upd, worst, co, len(to["ids"]), n_clones, dim
    return n_upd, worst, co, len(to["ids"])


def test_pipelined_driver_with_a_td_that_wanders_by_milliseconds(gpu_ctx):
    """Pipeline fuzz case 124 (tools/gpu/fuzz_pipeline.py): a fisheye camera publishing at 20 Hz from rest, 9-clone window - the camera-IMU
    time offset is poorly observable, sits still for dozens of updates and then steps by a millisecond.  Erase counts taken from the stale
    td were one IMU sample off (twice), two front-end frames integrated their gyro prediction over another window than the sequential
    loop's, and the runs parted.  With LVK_PIPE_TD_FACTOR=8 (read when the pipeline is created; the default 4 keeps bench.py's line where it
    was and REPORTS such counts) the caller's thread guesses less often: asked then is no unconfirmed count and equal bits."""
    import os
    os.environ["LVK_PIPE_TD_FACTOR"] = "8"
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver, VioPipeline
    from tests.conftest import synth_frames
    cam = dict(S.CAM_TUMVI_LIKE)
    frames = synth_frames(0, 200, cam=cam)
    seq = S.imu_only_sequence(cam=cam); ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(cam=cam, max_features_num=189, min_distance=25, pub_frequency=20)
    bcfg = S.backend_config(cam=cam, sw_size=9, if_fej=1, estimate_td=1, estimate_extrin=0, if_zupt_valid=0, aug_grid_rows=6, aug_grid_cols=6, max_features_in_one_grid=2,
                            max_track_len=8, pub_frequency=20)
    ctx2 = larvio_amd.Context(0); out = []
    for mode in ("seq", "pipe"):
        fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(bcfg, ctx2 if mode == "pipe" else gpu_ctx); assert be.initialize()
        drv = (VioPipeline if mode == "pipe" else VioDriver)(fe, be, imu_all)
        n_msg = 0
        for t, img in frames:
            r = drv.step(t, drv.visible_end(t), img=img); n_msg += int(r if mode == "pipe" else r[0])
        if mode == "pipe":
            drv.drain(); early, wrong = drv.early_counts()
            print("wandering td: %d messages, %d erase counts taken early, %d not confirmed; td %.2e" % (n_msg, early, wrong, be.state()["td"]))
            assert wrong == 0, (early, wrong)
            drv.close()
        out.append((n_msg, {k_: np.array(v, copy=True) for k_, v in be.state().items()}, be.cov(), be.counters(), fe.tracks()))
        be.close(); fe.close()
    ctx2.close(); del os.environ["LVK_PIPE_TD_FACTOR"]
    a, b = out
    assert a[0] == b[0] >= 150 and abs(a[1]["td"]) > 1e-3                      # the offset did wander (the true one is 0)
    for k_ in a[1]:
        assert np.array_equal(a[1][k_], b[1][k_]), k_
    assert np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4]["pts"], b[4]["pts"])


def test_driver_loop_config4_shape_equidistant_static_start_zupt(gpu_ctx):
    """512x512 equidistant camera, 300-feature budget, start at rest: static initialiser, ZUPT updates, then motion"""
    n_upd, worst, c, n_tracks = _driver_pair(gpu_ctx, TUMVI_LIKE, 0, 64, dict(max_features_num=300, min_distance=15),
                                             dict(sw_size=12, if_zupt_valid=1), init_from_gt=False, min_updates=15)
    assert c["zupt"] >= 1 and n_tracks > 60
    print("config-4 shape: updates", n_upd, "worst rel", worst, c, "tracks", n_tracks)


def test_driver_loop_blackout_noise_and_frozen_frames(gpu_ctx):
    """The whole loop through disturbances: a black frame (every track lost at once: one large MSCKF update, then a window without
    features), two frames of unrelated noise, and a camera that freezes for five frames while the IMU keeps moving (repeated image:
    zero parallax, the ZUPT test sees no feature motion).  The filter may well degrade — the oracle and the HIP path have to do so
    together."""
    n_upd, worst, c, n_tracks = _driver_pair(gpu_ctx, S_EUROC(), 40, 70, dict(max_features_num=150), dict(sw_size=20, if_zupt_valid=1),
                                             init_from_gt=True, min_updates=25, mutate=_disturb)
    print("disturbed run: updates", n_upd, "worst rel", worst, c, "tracks", n_tracks)


def test_driver_loop_headline_config_sw30(gpu_ctx):
    """BASELINE.json's metric configuration end to end against the oracle: 752x480, 150-feature budget, sw_size 30, 140 frames = 70
    messages, so the window fills (28 -> 30 clones cycle, larvio.cpp:2316-2320) and the pruning MSCKF update + re-anchoring run many
    times.  State and covariance within 1e-5 after EVERY update, ids / clone lists / gate counters identical."""
    n_upd, worst, c, n_tracks = _driver_pair(gpu_ctx, S_EUROC(), 40, 140, dict(max_features_num=150), dict(sw_size=30, max_features=150),
                                             init_from_gt=True, min_updates=60)
    assert c["msckf"] >= 5 and c["hybrid"] >= 55 and n_tracks >= 100, c
    print("headline config (sw_size 30): updates", n_upd, "worst rel", worst, c, "tracks", n_tracks)


def _oracle_threads():
    import os
    return min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1))


def test_whole_loop_configs1_as_benchmarked_150_live_tracks(gpu_ctx):
    """BASELINE.json configs[1] exactly as bench.py runs it (larvio_amd.synthetic.workload("A")): the tracker budget is sized so that
    the tracker HOLDS ~150 tracks, sw_size 30, 150 frames from t = 2 s: HIP vs oracle after every update."""
    from larvio_amd import synthetic as S
    wl = S.workload("A")
    n_upd, worst, c, n_tracks, n_clones, dim = _driver_pair(gpu_ctx, None, int(2.0 * wl["img_rate"]), 150, {}, {}, init_from_gt=True, min_updates=70, workload=wl)
    assert n_clones >= 28 and c["msckf"] >= 5 and 140 <= n_tracks <= wl["max_features"], (n_clones, c, n_tracks)
    print("configs[1] as benchmarked: updates", n_upd, "worst rel", worst, c, "tracks", n_tracks, "clones", n_clones, "dim", dim, "worst at", dict(_WORST_AT))


def test_whole_loop_configs2_imu_intrinsics_sw30(gpu_ctx):
    """configs[2]: online extrinsic + td + IMU-intrinsics calibration (46-dimensional legacy block, larvio.cpp:158-161, 3528-3800) as a
    WHOLE loop at sw_size 30: 140 frames, the window fills and cycles."""
    from larvio_amd import synthetic as S
    wl = S.workload("3")
    n_upd, worst, c, n_tracks, n_clones, dim = _driver_pair(gpu_ctx, None, int(2.0 * wl["img_rate"]), 140, {}, {}, init_from_gt=True, min_updates=65, workload=wl)
    assert wl["bcfg"]["calib_imu_instrinsic"] == 1 and n_clones >= 28 and c["msckf"] >= 5 and dim >= 46 + 6 * 28, (n_clones, c, dim)
    print("configs[2] (IMU intrinsics, sw 30): updates", n_upd, "worst rel", worst, c, "tracks", n_tracks, "clones", n_clones, "dim", dim, "worst at", dict(_WORST_AT))


def test_whole_loop_configs3_tumvi_300_tracks_sw30_zupt(gpu_ctx):
    """configs[3] at its real shape: 512x512 equidistant, ~300 live tracks (budget 350), sw_size 30, ZUPT on, starting AT REST: zero-velocity
    updates while the platform stands still, then motion; 170 frames so that the window fills (28 -> 30 cycle, larvio.cpp:2316-2320).
    The state is handed over at the second frame: with this many tracks the static initializer's 19th-largest-displacement test
    (StaticInitializer.cpp:60-75) never passes on this sequence - in the oracle either; the initializer itself is covered at a 300-feature
    budget by test_driver_loop_config4_shape_equidistant_static_start_zupt."""
    from larvio_amd import synthetic as S
    wl = S.workload("4")
    n_upd, worst, c, n_tracks, n_clones, dim = _driver_pair(gpu_ctx, None, 0, 170, {}, {}, init_from_gt=True, min_updates=60, workload=wl)
    assert n_clones >= 28 and c["zupt"] >= 1 and c["msckf"] >= 5 and n_tracks >= 200, (n_clones, c, n_tracks)
    print("configs[3] (300 tracks, sw 30, ZUPT): updates", n_upd, "worst rel", worst, c, "tracks", n_tracks, "clones", n_clones, "dim", dim, "worst at", dict(_WORST_AT))


def test_whole_loop_configs4_1080p_2000_tracks_sw60(gpu_ctx):
    """configs[4] at its real shape: 1920x1080 @60 Hz, 2000-feature budget, sw_size 60, 140 frames = 70 messages: the front-end at
    ~2000 tracks, the 58 -> 60 window cycle with pruning updates, and the tall-H compression (larvio.cpp:1430-1445: thousands of stacked
    rows per update) compared with the oracle after EVERY update."""
    from larvio_amd import synthetic as S
    wl = S.workload("5")
    n_upd, worst, c, n_tracks, n_clones, dim = _driver_pair(gpu_ctx, None, int(2.0 * wl["img_rate"]), 140, {}, {}, init_from_gt=True, min_updates=65,
                                                             workload=wl, oracle_threads=_oracle_threads())
    assert n_clones >= 58 and c["msckf"] >= 3 and n_tracks >= 1800 and dim >= 22 + 6 * 58, (n_clones, c, n_tracks, dim)
    print("configs[4] (1080p, 2000 tracks, sw 60): updates", n_upd, "worst rel", worst, c, "tracks", n_tracks, "clones", n_clones, "dim", dim, "worst at", dict(_WORST_AT))


def test_driver_loop_config5_shape_1080p_many_tracks(gpu_ctx):
    """1920x1080, 2000-feature budget, long window: capacities and the tall-H (QR compression) path at the largest configuration"""
    cam = dict(width=1920, height=1080, intrinsics=(1100.0, 1100.0, 960.0, 540.0), distortion_model=0,
               distortion=(-0.12, 0.03, 0.0002, -0.0001), T_cam_imu=None)
    import os
    n_upd, worst, c, n_tracks = _driver_pair(gpu_ctx, cam, 40, 14, dict(max_features_num=2000, min_distance=20),
                                             dict(sw_size=40, max_features_in_one_grid=2, if_zupt_valid=0, max_features=2000), init_from_gt=True, min_updates=5,
                                             oracle_threads=min(32, os.cpu_count() or 1))
    assert n_tracks > 600
    print("config-5 shape: updates", n_upd, "worst rel", worst, c, "tracks", n_tracks)


def test_pipelined_driver_is_identical_to_sequential_at_configs4_shape(gpu_ctx):
    """BASELINE.json configs[4] (1920x1080 @60 Hz, 2000 tracks, long window) through both drivers, three pipelined repeats: here the
    filter's launches share the GPU with heavy front-end kernels, workgroups of one launch start many microseconds apart, and any kernel
    whose workgroups read what a sibling overwrites shows up as a run-to-run difference (k_chol_left did, until round 2: the factored
    diagonal block went back into S while late workgroups still read A_pp from it; ~1 run in 5 diverged)."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver, VioPipeline
    wl = S.workload("5")
    n = 48
    first = int(2.0 * wl["img_rate"])
    ts, frames = S.render_frames(first, n + 1, cam=wl["cam"], seed=S.MASTER_SEED, img_rate=wl["img_rate"], procs=16)
    seq = S.imu_only_sequence(S.MASTER_SEED, cam=wl["cam"])
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    ctx2 = larvio_amd.Context(0)
    out = []
    for mode in ("seq", "pipe", "pipe", "pipe"):
        fe = larvio_amd.ImageProcessor(wl["fcfg"], gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(wl["bcfg"], ctx2 if mode == "pipe" else gpu_ctx); assert be.initialize()
        drv = (VioPipeline if mode == "pipe" else VioDriver)(fe, be, imu_all)
        for i in range(n):
            t = float(ts[i])
            if i == 1:
                if mode == "pipe":
                    drv.drain()
                k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
                t0 = imu_all["t"][k]; tr = seq.traj
                be.set_state(t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            drv.step(t, drv.visible_end(t), img=frames[i])
        if mode == "pipe":
            drv.drain(); drv.close()
        st = be.state()
        out.append(({k: np.array(v, copy=True) for k, v in st.items()}, be.cov(), be.counters(), fe.tracks()["ids"].copy()))
        be.close(); fe.close()
    ctx2.close()
    a = out[0]
    assert a[2]["hybrid"] >= 15 and a[2]["gated_in"] > 2000, a[2]
    for b in out[1:]:
        for k in a[0]:
            assert np.array_equal(a[0][k], b[0][k]), k
        assert np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_pipelined_driver_on_a_camera_off_the_imu_grid(gpu_ctx):
    """Every other pipelined-driver test feeds stamps that sit exactly on the synthetic grid, where lvk_vio_pipe_submit may ALWAYS take the
    IMU erase count early; a real camera is not aligned with the IMU.  Here the stamps carry a phase, per-frame jitter and jittered IMU
    times (larvio_amd.synthetic.unaligned_stamps), and td is estimated, so the bound "image time + td + half an IMU period"
    (larvio.cpp:464-512) wanders across IMU samples while the run goes on.  Asserted: some frames had to WAIT for their count
    (n_early < messages: the fall-back path ran on the GPU), no early count was found wrong, the pipelined run equals the sequential
    one bit for bit, and both agree with the oracle's loop on the same stamps (1e-5, discrete results identical)."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver, VioPipeline
    from oracle import lvo, lvo_be
    from tests.conftest import synth_frames
    frames = synth_frames(40, 120)
    seq = S.imu_only_sequence()
    ts0 = np.array([f[0] for f in frames])
    imu0 = seq.imu_array(max(int(ts0[0] * 200) - 4, 0), int(ts0[-1] * 200) + 40)
    ts, imu_all = S.unaligned_stamps(ts0, imu0)
    fcfg = S.frontend_config(max_features_num=150)
    bcfg = S.backend_config(sw_size=20, if_zupt_valid=0)
    k = int(np.searchsorted(imu_all["t"], ts[1], side="right")) - 1
    t0 = imu_all["t"][k]; tr = seq.traj
    init = (t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
    # ---- the oracle's loop
    ofe = lvo.Frontend(fcfg); obe = lvo_be.Ekf(bcfg)
    lo = 0; vis = lambda t: int(np.searchsorted(imu_all["t"], t + 0.05, side="left"))
    for i, (_, img) in enumerate(frames):
        if i == 1:
            obe.set_state(*init)
        buf = imu_all[lo:vis(ts[i])]
        have, m = ofe.process(img, float(ts[i]), buf)
        if have:
            _, used = obe.process(float(ts[i]), m, buf); lo += used
    ctx2 = larvio_amd.Context(0)
    out = []
    for mode in ("seq", "pipe"):
        fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(bcfg, ctx2 if mode == "pipe" else gpu_ctx); assert be.initialize()
        drv = (VioPipeline if mode == "pipe" else VioDriver)(fe, be, imu_all)
        n_msg = 0
        for i, (_, img) in enumerate(frames):
            if i == 1:
                if mode == "pipe":
                    drv.drain()
                be.set_state(*init)
            r = drv.step(float(ts[i]), drv.visible_end(float(ts[i])), img=img)
            n_msg += int(r if mode == "pipe" else r[0])
        if mode == "pipe":
            n_upd, n_m = drv.drain()
            early, wrong = drv.early_counts()
            assert n_m == n_msg and wrong == 0, (n_m, n_msg, early, wrong)
            assert 0 < early < n_msg - 4, ("the waiting path did not run" if early else "no count was ever taken early", early, n_msg)
            print("off-grid camera: %d messages, %d erase counts taken early (%d frames waited), %d wrong; td %.3e" % (n_m, early, n_m - early, wrong, be.state()["td"]))
            drv.close()
        st = be.state()
        out.append((n_msg, {k_: np.array(v, copy=True) for k_, v in st.items()}, be.cov(), be.clones()["id"].copy(), be.features()[0].copy(), be.counters(), fe.tracks()))
        be.close(); fe.close()
    ctx2.close()
    a, b = out
    assert a[0] == b[0] and a[0] >= 50
    for k_ in a[1]:
        assert np.array_equal(a[1][k_], b[1][k_]), k_
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5]
    for k_ in ("ids", "pts", "lifetime"):
        assert np.array_equal(a[6][k_], b[6][k_])
    so = obe.state()
    for k_ in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"):
        assert _rel(b[1][k_], so[k_]) < REL, k_
    assert abs(b[1]["td"] - so["td"]) < 1e-9 and abs(so["td"]) > 1e-6                 # td moved (the bound wandered), identically (where it stands at the end depends on which features are in the state: 4.8e-6 s with the reference's grid_map bookkeeping, 1.7e-5 before round 6)
    assert _rel(b[2], obe.cov()) < REL
    assert np.array_equal(b[3], obe.clones()["id"]) and np.array_equal(b[4], obe.features()[0])
    to = ofe.tracks()
    assert np.array_equal(b[6]["ids"], to["ids"]) and np.array_equal(b[6]["pts"], to["pts"])
    co = obe.counters()
    for k_ in ("hybrid", "msckf", "gated_in", "gated_out", "map"):
        assert b[5][k_] == co[k_], (k_, b[5], co)


def test_cpp_driver_matches_python_driver_bit_for_bit(gpu_ctx, tmp_path):
    """examples/larvio_main (C++ host classes of include/lvk_larvio.hpp, the loop of app/larvioMain.cpp:84-117) against the Python
    mirror driving the same library on the same sequence file contents: identical doubles."""
    import os, subprocess, sys
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver
    from tests.conftest import synth_frames
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s"])
    sys.path.insert(0, os.path.join(root, "examples"))
    from make_sequence import write_sequence
    frames = synth_frames(40, 50)
    path = str(tmp_path / "seq.bin")
    meta = write_sequence(path, frames=frames, max_features=150, sw_size=15)
    r = subprocess.run([os.path.join(root, "examples", "larvio_main"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = {l.split()[0]: l.split()[1:] for l in r.stdout.strip().splitlines()}
    cpp_state = np.array([float(x) for x in lines["state"]])
    # the same loop through the Python mirror (host images, one context)
    fe = larvio_amd.ImageProcessor(S.frontend_config(max_features_num=150), gpu_ctx); assert fe.initialize()
    be = larvio_amd.LarVio(S.backend_config(sw_size=15, if_zupt_valid=0), gpu_ctx); assert be.initialize()
    imu_all = meta["imu"]
    drv = VioDriver(fe, be, imu_all)
    n_msgs = n_upd = 0
    for i, (t, img) in enumerate(frames):
        if i == meta["init_frame"]:
            x = meta["init"]
            be.set_state(x[0], x[1:5], x[5:8], x[8:11], x[11:14], x[14:17], x[17:20], x[20:23])
        has, upd = drv.step(t, drv.visible_end(t), img=img)
        n_msgs += int(has); n_upd += int(upd)
    assert [int(lines["frames"][0]), int(lines["frames"][2]), int(lines["frames"][4]), int(lines["frames"][6])] == [len(frames), n_msgs, n_upd, be.dim]
    s = be.state()
    py_state = np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]])
    assert np.array_equal(cpp_state, py_state)
    assert n_upd >= 15
    be.close(); fe.close()


def test_cpp_dataset_driver_on_an_asl_directory(gpu_ctx, tmp_path):
    """examples/larvio_euroc — the reference's command line (app/larvioMain.cpp:27-31): IMU csv, image csv, image directory,
    configuration file — on the synthetic sequence written as an ASL/EuRoC directory (PNG files, CRLF csv, OpenCV-style YAML).
    Starts at rest (static initializer).  The trajectory it logs must equal, double for double, what the Python mirror produces
    from the same stamps and pixels; the reference's own two log files (larvio.cpp:388,446-453) must be there as well."""
    import os, subprocess, sys
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver
    from tests.conftest import synth_frames
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(root, "examples"), "-s"])
    sys.path.insert(0, os.path.join(root, "examples")); sys.path.insert(0, os.path.join(root, "tools"))
    from make_euroc_dir import write_euroc_dir, rot_to_quat_wxyz
    import traj_rmse
    cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
    frames = synth_frames(0, 64, cam=cam)                       # the frames of the config-4 test above (cached)
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
    bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
    out_dir = str(tmp_path / "logs") + "/"; os.makedirs(out_dir)
    d = str(tmp_path / "seq")
    gt = [(t, seq.traj.p_wb(t), rot_to_quat_wxyz(seq.traj.R_wb(t))) for t in np.arange(ts[0], ts[-1] + 0.0051, 0.005)]
    t_img, t_imu = write_euroc_dir(d, frames, imu_all, fcfg, bcfg, ground_truth=gt, output_dir=out_dir)
    tum = str(tmp_path / "traj.txt")
    r = subprocess.run([os.path.join(root, "examples", "larvio_euroc"), d + "/mav0/imu0/data.csv", d + "/mav0/cam0/data.csv", d + "/mav0/cam0/data",
                        d + "/config.yaml", "--tum", tum], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    cpp = np.loadtxt(tum, ndmin=2)
    # --pipelined: lvk::VioPipeline (filter on its own stream and thread, odometry through the callback) — the same numbers
    seq_log = open(out_dir + "msckf_2_state.txt").read()
    tum2 = str(tmp_path / "traj_pipelined.txt")
    r2 = subprocess.run(r.args[:-2] + ["--tum", tum2, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    print(r2.stdout)
    assert open(tum2).read() == open(tum).read() and open(out_dir + "msckf_2_state.txt").read() == seq_log
    assert r2.stdout.splitlines()[0] == r.stdout.splitlines()[0]
    # the ADAPTER (adapter/: larvio::ImageProcessor / larvio::LarVio with the reference's exact signatures, cv::Mat / Eigen / boost
    # from stub headers) driven by the loop of app/larvioMain.cpp:84-117: the same positions, and every getter the reference's
    # drivers call answers (getPpose / getPvel / getSwPoses / both map-point getters / getVisualImg)
    subprocess.check_call(["make", "-C", os.path.join(root, "adapter"), "-s"])
    tum3 = str(tmp_path / "traj_adapter.txt")
    r3 = subprocess.run([os.path.join(root, "adapter", "adapter_main")] + r.args[1:5] + ["--tum", tum3], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    print(r3.stdout)
    ad = np.loadtxt(tum3, ndmin=2)
    assert ad.shape[0] == cpp.shape[0] and np.array_equal(ad[:, 1:4], cpp[:, 1:4])
    # the adapter defers processFeatures by default (lvk_ekf_process_async; getters wait): LVK_ADAPTER_BLOCKING=1 = the blocking call,
    # every number printed must be the same
    tum4 = str(tmp_path / "traj_adapter_blocking.txt")
    r4 = subprocess.run(r3.args[:-1] + [tum4], capture_output=True, text=True, timeout=300, env=dict(os.environ, LVK_ADAPTER_BLOCKING="1"))
    assert r4.returncode == 0, r4.stdout + r4.stderr
    assert open(tum4).read() == open(tum3).read()
    assert (ad[:, 7] > 0).all() and (ad[:, 8] > 0).all()                        # P_pose(0,0) = position variance, P_vel(0,0)
    assert ad[-1, 9] >= 5 and (ad[:, 10] == 512 * 512 * 3).all()                # sliding-window poses; RGB visual image of the right size
    assert f"odometry updates {cpp.shape[0]}" in r3.stdout
    # the same loop through the Python mirror, on the stamps as the readers deliver them (1e-9 * integer ns)
    fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
    be = larvio_amd.LarVio(dict(bcfg, max_features=300), gpu_ctx); assert be.initialize()
    imu2 = imu_all.copy(); imu2["t"] = t_imu
    drv = VioDriver(fe, be, imu2)
    rows = []
    for t, (_, img) in zip(t_img, frames):
        hi = int(np.count_nonzero(t_imu - float(t) < 0.05))     # the driver's own predicate (larvioMain.cpp:99), rounding included
        has, upd = drv.step(float(t), hi, img=img)
        if upd:
            s = be.state(); rows.append(np.concatenate([[s["t"]], s["p"], s["q"]]))
    py = np.array(rows)
    assert len(py) >= 15 and cpp.shape == py.shape
    assert np.array_equal(cpp[:, 1:], py[:, 1:]) and np.abs(cpp[:, 0] - py[:, 0]).max() < 1e-8          # stamps are printed with 9 decimals
    # the reference's logs
    log = np.loadtxt(out_dir + "msckf_2_state.txt", ndmin=2)
    t0 = float(open(out_dir + "msckf_2_takeoff.txt").read())
    assert log.shape == (len(py), 24) and abs(t0 - be.take_off_stamp) < 1e-8
    assert np.allclose(log[:, 0] + t0, py[:, 0], atol=1e-4) and np.allclose(log[:, 8:11], py[:, 1:4], rtol=1e-5, atol=1e-6)
    assert np.allclose(log[:, [2, 3, 4, 1]], py[:, 4:8], rtol=1e-5, atol=1e-6)
    # and the error tool on both forms of the output
    t_gt, p_gt = traj_rmse.load_trajectory(d + "/mav0/state_groundtruth_estimate0/data.csv")
    e1, n1 = traj_rmse.ate_rmse(cpp[:, 0], cpp[:, 1:4], t_gt, p_gt)
    tl, pl = traj_rmse.load_trajectory(out_dir + "msckf_2_state.txt")
    e2, n2 = traj_rmse.ate_rmse(tl, pl, t_gt, p_gt)
    print("ATE RMSE", e1, e2, "poses", n1)
    # (3 s from rest with a slow ramp: the algorithm's own ZUPT holds the velocity at zero into the start of the motion, so the absolute
    #  error is large here for the oracle and the HIP path alike; what is asserted is that the two forms of the log agree)
    assert n1 == n2 == len(py) and e1 < 1.0 and abs(e1 - e2) < 1e-3
    be.close(); fe.close()
    # BASELINE.json's trajectory clause, on the data at hand: the CPU oracle over the same files' contents, RMSE within 1 mm
    from oracle import lvo, lvo_be
    ofe = lvo.Frontend(fcfg); obe = lvo_be.Ekf(bcfg)
    lo = 0; rows = []
    for t, (_, img) in zip(t_img, frames):
        hi = int(np.count_nonzero(t_imu - float(t) < 0.05))
        have, m = ofe.process(img, float(t), imu2[lo:hi])
        if have:
            upd, used = obe.process(float(t), m, imu2[lo:hi]); lo += used
            if upd:
                so = obe.state(); rows.append(np.concatenate([[so["t"]], so["p"]]))
    orc = np.array(rows)
    assert orc.shape[0] == len(py)
    e3, n3 = traj_rmse.ate_rmse(orc[:, 0], orc[:, 1:4], t_gt, p_gt)
    print("ATE RMSE: HIP %.6f m, CPU oracle %.6f m, difference %.4f mm; largest position difference %.3e m"
          % (e1, e3, 1e3 * (e1 - e3), np.abs(orc[:, 1:4] - py[:, 1:4]).max()))
    assert abs(e1 - e3) < 1e-3
