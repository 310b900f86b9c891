"""Probe of the global ORB search (lvk_orb_match_global) for a kernel trace and for host wall times.

    python tools/gpu/orb_global_probe.py kernels      six calls each at 4096 corners x 65,536 and x 1,048,576 map points, and six calls of the
                                                      guided matcher at 1024 queries x 4096 corners with an infinite radius - the yardstick of
                                                      DESIGN.md 5.0h; run it behind `rocprofv3 --kernel-trace --stats --` for the medians
    python tools/gpu/orb_global_probe.py wall         wall time of ImageProcessor.relocalise_map at 752 x 480 with a 1,048,576-point map, and of
                                                      one match_landmarks call with 1024 queries and an infinite radius (what covering that
                                                      map took before, 1024 times over)
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import larvio_amd                                             # noqa: E402
from larvio_amd import ops, synthetic as S                    # noqa: E402
from larvio_amd._lib import MAP_MAX_POINTS                    # noqa: E402


def kernels():
    ctx = larvio_amd.Context(0)
    rng = np.random.default_rng(1)
    md = rng.integers(0, 256, (MAP_MAX_POINTS, 32), dtype=np.uint8)
    src = rng.integers(0, 65536, 4096)
    cd = md[src].copy(); cd[:, :4] ^= rng.integers(0, 256, (4096, 4), dtype=np.uint8)       # ~16 bits off a map point of the first 65,536
    d_map = ctx.to_device(md)
    out = {}
    for n_map in (65536, MAP_MAX_POINTS):
        for _ in range(6):
            r = ops.orb_match_global(ctx, (d_map, n_map), cd, ratio_pct=80)
        out[f"n_ok_{n_map}"] = int(r["info"]["n_ok"])
    pts = np.stack([rng.integers(0, 752, 4096), rng.integers(0, 480, 4096)], -1).astype(np.float32)
    for _ in range(6):
        g = ops.orb_match_guided(ctx, pts, md[:4096], np.full((1024, 2), 100.0, np.float32), np.inf, cd[:1024])
    out["guided_n_window"] = int(g["n_window"][0])
    ctx.close()
    return out


def wall():
    cfg = S.frontend_config()
    seq = S.Sequence()
    gpu = larvio_amd.ImageProcessor(cfg)
    assert gpu.initialize()
    t_prev = None
    for i in range(3):
        ts, img = seq.frame(i)
        k0, k1 = seq.imu_index_range(ts - 1.0 if t_prev is None else t_prev, ts)
        gpu.processImage(img, seq.imu_array(k0, k1), ts=ts)
        t_prev = ts
    # the map: the frame's own corners and descriptors (ops' stage entries on the same image, as the front-end detects them), lifted to 3D at
    # arbitrary depths through the camera pose, first; uniformly random descriptors at random positions behind them - so that the timed calls
    # select, gather, draw 4096 pairs and score them, not only search
    rng = np.random.default_rng(2)
    n = MAP_MAX_POINTS
    ctx = gpu.ctx
    pyr = ops.Pyramid(ctx, cfg["width"], cfg["height"], cfg["patch_size"], cfg["pyramid_levels"]).build(img, clahe=bool(cfg["flag_equalize"]))
    pts = ops.good_features_from_map(ctx, pyr.min_eigen_map(), 4096, 0.01, float(cfg["min_distance"]), cap=4096)
    pyr.orb_prepare()
    desc, _ = ops.orb_describe(ctx, pyr, pts)
    und = ops.undistort(ctx, pts, cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], (1.0, 1.0, 0.0, 0.0)).reshape(-1, 2).astype(np.float64)
    R_wc, p_wc = seq.traj.cam_pose(t_prev)
    z = rng.uniform(2.0, 9.0, len(pts))
    X = rng.uniform(-30, 30, (n, 3)); X[:len(pts)] = np.column_stack([und * z[:, None], z]) @ np.asarray(R_wc).T + np.asarray(p_wc)
    md = rng.integers(0, 256, (n, 32), dtype=np.uint8); md[:len(pts)] = desc
    gpu.set_map(X, None, md)
    reloc = []
    for _ in range(6):
        t0 = time.perf_counter()
        res, m, info = gpu.relocalise_map(R_wc, p_wc, ratio_pct=80)
        reloc.append(time.perf_counter() - t0)
    q = np.full((1024, 2), 100.0, np.float32); qd = rng.integers(0, 256, (1024, 32), dtype=np.uint8)
    one = []
    for _ in range(6):
        t0 = time.perf_counter()
        gpu.match_landmarks(q, np.inf, qd, ratio_pct=80)
        one.append(time.perf_counter() - t0)
    out = dict(relocalise_map_ms=[round(1e3 * t, 3) for t in reloc], match_landmarks_1024_ms=[round(1e3 * t, 3) for t in one], corners=int(gpu.last_match_candidates),
               n_ok=int(info["n_ok"]), n_selected=int(info["n_selected"]), align_status=int(res["status"]), n_inliers=int(res["n_inliers"]), map_points=n)
    gpu.close()
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    print(json.dumps({"mode": mode, **(kernels() if mode == "kernels" else wall())}))
