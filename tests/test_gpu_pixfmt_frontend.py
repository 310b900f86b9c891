"""GPU: the front-end's input pixel formats (lvk_frontend_set_input_format) through the C ABI and the Python classes.

The judge is the front-end itself on its default path: front-end A is fed colour / 16-bit / YUV frames, front-end B the MONO8 frames
tests/pixfmt_ref.py makes of them (the numpy restatement of include/lvk_c.h); after EVERY frame tracks, new points and the feature
message must be byte-identical.  Resolution: the 301 x 203 window of tests/mask_replay.py, the smallest the front-end's edge tests run
(300 x 203 for the two YUV layouts, which need an even width)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mask_replay as MR
from tests import pixfmt_ref as PR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LVK_ERR_ARG = 1
N_FRAMES = 12
NON_DEFAULT = PR.FORMATS[1:]


def _small(fmt, n=N_FRAMES):
    """-> (grey frames [(ts, img)], imu sequence, front-end configuration) at the smallest resolution `fmt` can have"""
    frames, seq, cfg = MR.sequence("odd")
    frames = frames[:n]
    if fmt in ("yuyv", "uyvy"):
        cfg = dict(cfg, width=cfg["width"] - 1)
        frames = [(t, np.ascontiguousarray(img[:, :-1])) for t, img in frames]
    return frames, seq, cfg


def _snapshot(fe, have, msg):
    tr = fe.tracks()
    return (bool(have), msg.features.tobytes() if have else b"", fe.new_pts().tobytes(), fe.state) + tuple(tr[k].tobytes() for k in ("ids", "pts", "lifetime", "init", "desc"))


def _feed(fe, ctx, img, imu, ts, fmt, route, keep):
    """one frame of format `fmt` into `fe`: route 'host' = a contiguous host array, 'host-padded' = a window of a wider host array
    (padded row stride), 'device' = a device pointer into a larger allocation, rows padded"""
    if route == "host":
        return fe.processImage(img, imu, ts=ts)
    h, w = img.shape[:2]
    row = w * PR.BPP[fmt]
    raw = np.ascontiguousarray(img).view(np.uint8).reshape(h, row)
    if route == "host-padded":
        extra = 3 if fmt != "mono16" else 4                  # pixels of the wider array
        big = np.full((h, w + extra) + img.shape[2:], 0x5A, img.dtype)
        big[:, 1:1 + w] = img
        view = big[:, 1:1 + w]
        assert view.strides[0] == (w + extra) * PR.BPP[fmt]
        return fe.processImage(view, imu, ts=ts)
    assert route == "device"
    base, pad = (2, 6) if fmt == "mono16" else (1, 13)       # mono16: even address and stride; the others: an odd address, any stride
    host = np.full(base + h * (row + pad), 0x5A, np.uint8)
    for y in range(h):
        host[base + y * (row + pad): base + y * (row + pad) + row] = raw[y]
    buf = ctx.to_device(host)
    keep.append(buf)                                         # the image stage reads it asynchronously: freed after the run
    return fe.processImage(None, imu, ts=ts, device_ptr=buf.ptr + base, stride=row + pad)


def _twin_run(ctx, fmt, route, shift=0):
    """front-end A on `fmt` frames over `route` against front-end B on their MONO8 conversion; -> frames compared"""
    import larvio_amd
    frames, seq, cfg = _small(fmt)
    rng = np.random.default_rng(PR.CODE[fmt])
    a = larvio_amd.ImageProcessor(cfg, ctx); b = larvio_amd.ImageProcessor(cfg, ctx)
    assert a.initialize() and b.initialize()
    assert a.input_format == "mono8"
    a.set_input_format(fmt, shift)
    assert a.input_format == fmt and b.input_format == "mono8"
    keep = []
    n_msg = 0
    for i, (ts, grey) in enumerate(frames):
        img = PR.from_gray(rng, grey, fmt, shift)
        want_grey = PR.to_gray(img, fmt, shift)
        imu = MR.imu_for(seq, ts)
        ha, ma = _feed(a, ctx, img, imu, ts, fmt, route, keep)
        hb, mb = b.processImage(want_grey, imu, ts=ts)
        sa, sb = _snapshot(a, ha, ma), _snapshot(b, hb, mb)
        assert sa == sb, (fmt, route, i, [x == y for x, y in zip(sa, sb)])
        n_msg += int(ha)
    n_tracks = len(a.tracks()["ids"])
    a.close(); b.close()
    for buf in keep:
        buf.free()
    assert n_msg >= 3 and n_tracks > 10, (n_msg, n_tracks)   # not vacuous: messages were published and the tracker lives
    return len(frames)


@pytest.mark.parametrize("route", ["host", "host-padded", "device"])
@pytest.mark.parametrize("fmt", NON_DEFAULT)
def test_twin_front_ends_are_byte_identical(gpu_ctx, fmt, route):
    assert _twin_run(gpu_ctx, fmt, route, shift=4 if fmt == "mono16" else 0) == N_FRAMES


def test_twin_front_ends_on_the_pinned_staging_route():
    """LVK_BAR_PUSH=0 sends a blocking caller's host images through the pinned staging ring and the copy engine.  The library decides
    that once per process and device (lvk_bar_usable), and this process decided long ago: the switch only means something in a process
    that starts with it, so the twins of every format run in a fresh one."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import larvio_amd\n"
            "from tests import test_gpu_pixfmt_frontend as T\n"
            "ctx = larvio_amd.Context()\n"
            "for fmt in T.NON_DEFAULT:\n"
            "    for route in ('host', 'host-padded'):\n"
            "        T._twin_run(ctx, fmt, route, shift=4 if fmt == 'mono16' else 0)\n"
            "ctx.close()\n"
            "print('pinned twins ok')\n" % ROOT)
    env = dict(os.environ, LVK_BAR_PUSH="0", LVK_VERBOSE="1")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + ["-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pinned twins ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "LVK_BAR_PUSH=0: staging through pinned host memory" in r.stderr, r.stderr[-2000:]


def test_switching_back_to_mono8_is_the_all_grey_run(gpu_ctx):
    import larvio_amd
    frames, seq, cfg = _small("bgr8")
    rng = np.random.default_rng(11)
    a = larvio_amd.ImageProcessor(cfg, gpu_ctx); b = larvio_amd.ImageProcessor(cfg, gpu_ctx)
    assert a.initialize() and b.initialize()
    from larvio_amd._lib import lib
    L = lib()
    assert L.lvk_frontend_input_format(a._h) == PR.CODE["mono8"]
    a.set_input_format("bgr8")
    assert L.lvk_frontend_input_format(a._h) == PR.CODE["bgr8"]
    for i, (ts, grey) in enumerate(frames):
        if i == 6:
            a.set_input_format("mono8")
            assert L.lvk_frontend_input_format(a._h) == PR.CODE["mono8"] and a.input_format == "mono8"
        imu = MR.imu_for(seq, ts)
        if i < 6:
            img = PR.from_gray(rng, grey, "bgr8"); g = PR.to_gray(img, "bgr8")
            ha, ma = a.processImage(img, imu, ts=ts)
        else:
            g = grey
            ha, ma = a.processImage(grey, imu, ts=ts)
        hb, mb = b.processImage(g, imu, ts=ts)
        assert _snapshot(a, ha, ma) == _snapshot(b, hb, mb), i
    assert len(a.tracks()["ids"]) > 10
    a.close(); b.close()
    assert L.lvk_frontend_input_format(None) == -1 and L.lvk_frontend_set_input_format(None, 1, 0) == LVK_ERR_ARG


def test_pipelined_driver_fed_bgr8_is_the_run_fed_its_grey(gpu_ctx):
    """VioPipeline at the headline configuration's shape (752 x 480, 150-feature budget, sw_size 30) over a short window: BGR8 frames
    in one run, their conversion in the other; state, covariance, id lists, counters and tracks after the drain are array_equal."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioPipeline
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import _R2q
    frames = synth_frames(40, 70)[:30]
    rng = np.random.default_rng(21)
    colour = [PR.from_gray(rng, img, "bgr8") for _, img in frames]
    grey = [PR.to_gray(c, "bgr8") for c in colour]
    seq = S.imu_only_sequence()
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(max_features_num=150)
    bcfg = S.backend_config(sw_size=30, max_features=150)
    ctx2 = larvio_amd.Context(0)
    out = []
    for fmt, imgs in (("bgr8", colour), ("mono8", grey)):
        fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
        be = larvio_amd.LarVio(bcfg, ctx2); assert be.initialize()
        if fmt != "mono8":
            fe.set_input_format(fmt)                         # before the first submit
        drv = VioPipeline(fe, be, imu_all)
        n_msg = 0
        for i, t in enumerate(ts):
            if i == 1:
                drv.drain()
                k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
                t0 = imu_all["t"][k]; tr = seq.traj
                be.set_state(t0, _R2q(tr.R_wb(t0)), tr.p_wb(t0), tr.vel(t0), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
            n_msg += int(drv.step(t, drv.visible_end(t), img=imgs[i]))
        n_upd, n_m = drv.drain()
        assert n_m == n_msg
        drv.close()
        st = be.state()
        out.append((n_msg, n_upd, be.dim, {k: np.array(v, copy=True) for k, v in st.items()}, be.cov(), be.clones()["id"].copy(), be.features()[0].copy(),
                    be.counters(), fe.tracks()))
        be.close(); fe.close()
    ctx2.close()
    a, b = out
    assert a[0] == b[0] >= 10 and a[1] == b[1] >= 5 and a[2] == b[2]
    for k in a[3]:
        assert np.array_equal(a[3][k], b[3][k]), k
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and np.array_equal(a[6], b[6]) and a[7] == b[7]
    for k in ("ids", "pts", "lifetime", "init", "desc"):
        assert np.array_equal(a[8][k], b[8][k]), k
    assert len(a[8]["ids"]) > 60


def test_front_end_refusals(gpu_ctx):
    import larvio_amd
    from larvio_amd._lib import lib, Image, IMU, OBS
    L = lib()
    frames, seq, cfg = _small("bgr8")                        # 301 x 203: an odd width
    w, h = cfg["width"], cfg["height"]
    rng = np.random.default_rng(31)
    a = larvio_amd.ImageProcessor(cfg, gpu_ctx); b = larvio_amd.ImageProcessor(cfg, gpu_ctx)
    assert a.initialize() and b.initialize()
    a.set_input_format("bgr8")
    # YUV on an odd configured width, an unknown format, a bad shift: refused, and bgr8 stays in force
    for fmt, shift in ((PR.CODE["yuyv"], 0), (PR.CODE["uyvy"], 0), (8, 0), (-1, 0), (PR.CODE["mono16"], 9), (PR.CODE["mono16"], -1), (PR.CODE["rgb8"], 2), (PR.CODE["mono8"], 1)):
        assert L.lvk_frontend_set_input_format(a._h, fmt, shift) == LVK_ERR_ARG, (fmt, shift)
        assert L.lvk_frontend_input_format(a._h) == PR.CODE["bgr8"]
    with pytest.raises(larvio_amd.LvkError, match="even width"):
        a.set_input_format("yuyv")
    with pytest.raises(ValueError):
        a.set_input_format("bayer")
    assert a.input_format == "bgr8"
    out = np.zeros(cfg["max_features_num"], OBS)
    for i, (ts, grey) in enumerate(frames):
        img = PR.from_gray(rng, grey, "bgr8")
        imu = np.ascontiguousarray(MR.imu_for(seq, ts), IMU)
        if i in (0, 5):                                      # before the first-image gate and in steady state
            n, has = C.c_int(0), C.c_int(0)
            im = Image(img.ctypes.data, w, h, 3 * w - 1, 0)  # a stride below width * bytes_per_pixel
            st = L.lvk_frontend_process(a._h, C.byref(im), float(ts), imu.ctypes.data_as(C.c_void_p), len(imu), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), C.byref(has))
            assert st == LVK_ERR_ARG and b"bgr8" in L.lvk_last_error(gpu_ctx.h)
            im = Image(img.ctypes.data, w, h, w, 0)          # what a MONO8 caller would pass
            st = L.lvk_frontend_process(a._h, C.byref(im), float(ts), imu.ctypes.data_as(C.c_void_p), len(imu), out.ctypes.data_as(C.c_void_p), len(out), C.byref(n), C.byref(has))
            assert st == LVK_ERR_ARG
            with pytest.raises(ValueError, match="bgr8"):    # Python: a 2-D uint8 array under bgr8
                a.processImage(grey, imu, ts=ts)
            with pytest.raises(ValueError, match="bgr8"):
                a.processImage(img.view(np.uint8).reshape(h, 3 * w).view(np.uint16) if (3 * w) % 2 == 0 else img[..., :2], imu, ts=ts)
        ha, ma = a.processImage(img, imu, ts=ts)             # the next good frame is processed: the twin never saw the refusals
        hb, mb = b.processImage(PR.to_gray(img, "bgr8"), imu, ts=ts)
        assert _snapshot(a, ha, ma) == _snapshot(b, hb, mb), i
    assert len(a.tracks()["ids"]) > 10
    a.close(); b.close()


def test_adapter_fed_other_formats_prints_the_default_run(tmp_path):
    """adapter/adapter_main --input-format: larvio::ImageProcessor::setInputFormat, then every frame as a 3-channel (or 16-bit) cv::Mat
    whose grey is the decoded frame.  Trajectory log, counts and the size of getVisualImg's picture equal the default run's."""
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "adapter"), "-s"])
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from make_euroc_dir import write_euroc_dir
    cam = dict(S.CAM_TUMVI_LIKE)
    frames = synth_frames(0, 64, cam=cam)
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
    bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
    d = str(tmp_path / "seq")
    out_dir = str(tmp_path / "logs") + "/"; os.makedirs(out_dir)
    write_euroc_dir(d, frames, imu_all, fcfg, bcfg, output_dir=out_dir)
    args = [os.path.join(ROOT, "adapter", "adapter_main"), d + "/mav0/imu0/data.csv", d + "/mav0/cam0/data.csv", d + "/mav0/cam0/data", d + "/config.yaml"]
    runs = {}
    for name in ("mono8", "bgr8", "mono16:8"):
        tum = str(tmp_path / ("traj_%s.txt" % name.replace(":", "_")))
        r = subprocess.run(args + ["--tum", tum] + ([] if name == "mono8" else ["--input-format", name]), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = (open(tum).read(), r.stdout.strip().splitlines()[-1])
    rows = np.loadtxt(str(tmp_path / "traj_mono8.txt"), ndmin=2)
    assert rows.shape[0] >= 10 and (rows[:, 10] == 512 * 512 * 3).all()
    assert runs["bgr8"] == runs["mono8"] and runs["mono16:8"] == runs["mono8"]
    r = subprocess.run(args + ["--input-format", "mono16:9"], capture_output=True, text=True, timeout=300)      # a refusal reaches the caller
    assert r.returncode == 1 and "setInputFormat" in r.stdout and "refused" in r.stderr
