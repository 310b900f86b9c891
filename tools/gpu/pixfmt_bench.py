"""What the input pixel formats cost (lvk_image_to_gray, lvk_frontend_set_input_format); DESIGN.md 5.0b, profiles/pixfmt_*.

  python tools/gpu/pixfmt_bench.py [--out FILE] [--launches 300] [--reps 3]

1. The conversion kernel alone: HIP events around `--launches` back-to-back launches on the context's stream, per format, at 752 x 480
   and 1920 x 1080 (source rows tightly packed and aligned, the front-end's own layout).  us per launch and the bytes it moves per second.
2. The pipelined driver (VioPipeline) at the headline configuration's shape over 140 synthetic frames, host images: fed BGR8 against fed
   the pre-converted grey, alternating, `--reps` runs each; frames/s over the last 100 frames, drain included.  The difference is the
   price of the format: wider staging copy, wider H2D, one launch.
No host-side conversion is timed here."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FORMATS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "mono16", "yuyv", "uyvy")


def kernel_times(ctx, launches, say):
    import ctypes as C
    import torch
    from larvio_amd._lib import lib, PIX_FORMATS, pixfmt_bytes_per_pixel
    L = lib()
    stream = torch.cuda.ExternalStream(ctx.stream)
    rng = np.random.default_rng(0)
    for w, h in ((752, 480), (1920, 1080)):
        for fmt in FORMATS:
            bpp = pixfmt_bytes_per_pixel(fmt)
            src = ctx.to_device(rng.integers(0, 256, w * h * bpp, dtype=np.uint8)); dst = ctx.alloc(w * h)
            args = (ctx.h, C.c_void_p(src.ptr), w * bpp, w, h, PIX_FORMATS[fmt], 0, C.c_void_p(dst.ptr), w)
            for _ in range(20):
                ctx.check(L.lvk_image_to_gray(*args))
            ctx.sync()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(launches):
                L.lvk_image_to_gray(*args)
            b.record(stream)
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / launches
            say("kernel %-6s %4dx%-4d  %7.2f us/launch  %7.1f GB/s (%d launches between two events)" % (fmt, w, h, us, w * h * (bpp + 1) / us * 1e-3, launches))
            src.free(); dst.free()


def pipeline_fps(ctx, ctx2, fmt, frames_in, imu_all, seq, fcfg, bcfg, timed=100):
    import larvio_amd
    from larvio_amd.vio import VioPipeline
    from larvio_amd.synthetic import R2q
    fe = larvio_amd.ImageProcessor(fcfg, ctx); assert fe.initialize()
    be = larvio_amd.LarVio(bcfg, ctx2); assert be.initialize()
    if fmt != "mono8":
        fe.set_input_format(fmt)
    drv = VioPipeline(fe, be, imu_all)
    ends = [drv.visible_end(t) for t, _ in frames_in]
    t0 = None
    for i, (t, img) in enumerate(frames_in):
        if i == 1:
            drv.drain()
            k = int(np.searchsorted(imu_all["t"], t, side="right")) - 1
            ti = imu_all["t"][k]; tr = seq.traj
            be.set_state(ti, R2q(tr.R_wb(ti)), tr.p_wb(ti), tr.vel(ti), np.zeros(3), np.zeros(3), imu_all["gyro"][k], imu_all["acc"][k])
        if i == len(frames_in) - timed:
            drv.drain(); t0 = time.perf_counter()
        drv.step(t, ends[i], img=img)
    drv.drain()
    dt = time.perf_counter() - t0
    drv.close(); be.close(); fe.close()
    return timed / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    import larvio_amd
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    from tests import pixfmt_ref as PR
    frames = synth_frames(40, 140)                           # rendered in a child process BEFORE this one touches the GPU
    ctx = larvio_amd.Context(0); ctx2 = larvio_amd.Context(0)
    kernel_times(ctx, a.launches, say)
    rng = np.random.default_rng(1)
    colour = [(t, PR.from_gray(rng, img, "bgr8")) for t, img in frames]
    grey = [(t, PR.to_gray(img, "bgr8")) for t, img in colour]
    seq = S.imu_only_sequence()
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(max_features_num=150); bcfg = S.backend_config(sw_size=30, max_features=150)
    pipeline_fps(ctx, ctx2, "mono8", grey, imu_all, seq, fcfg, bcfg)                    # warm-up, not reported
    res = {"mono8": [], "bgr8": []}
    for r in range(a.reps):
        for fmt, fr in (("mono8", grey), ("bgr8", colour)):
            res[fmt].append(pipeline_fps(ctx, ctx2, fmt, fr, imu_all, seq, fcfg, bcfg))
            say("pipeline 752x480 host images, fed %-5s run %d: %8.1f frames/s (last 100 of 140 frames, drain included)" % (fmt, r + 1, res[fmt][-1]))
    m8, mc = float(np.mean(res["mono8"])), float(np.mean(res["bgr8"]))
    say("pipeline means: grey %.1f frames/s, bgr8 %.1f frames/s: %+.1f %% (%.1f us per frame)" % (m8, mc, 100 * (mc / m8 - 1), 1e6 / mc - 1e6 / m8))
    ctx2.close(); ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
