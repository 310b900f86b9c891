"""The case table of the prior-map selection tests (CPU only: inputs).  tests/test_map_select_ref.py holds the restatement
(tests/map_select_ref.py) to a plain loop, to the long-double judge and to larvio_amd.localize on every case;
tests/test_gpu_map_select_stages.py runs the same cases on the GPU against the restatement - one table, so the two cannot drift.

Margins.  The discrete fields (status, cell, hence the selection) are thresholds on FP64 values: a pixel against an image or cell border, a
depth against min_depth / max_depth, r2 against max_r2.  The FP64 chain is ~40 operations on values of order 1 (normalised coordinates) to
10^3 (pixels), so its error is of order 40 x 2^-53 x 10^3 ~ 4e-12 px (and ~1e-14 m in depth; atan is within an ulp in any libm) - five
orders below PIX_MARGIN = 1e-6 px and DEPTH_MARGIN = 1e-9.  Every random case is built so that no point lies closer than that to a
threshold (a point that does is moved behind the camera), so each discrete field has one right value whatever the last bits are;
tests/test_map_select_ref.py asserts it against the judge.  The deliberate edge cases (exact=True) sit ON thresholds instead and use
numbers that make every operation exact."""
import functools

import numpy as np

from tests import map_select_ref as R

PIX_MARGIN, DEPTH_MARGIN = 1e-6, 1e-9
CHUNK = 256                    # points per workgroup of the kernels (larvio_amd/csrc/fe_map.hip)

CAM_RADTAN = dict(width=752, height=480, intrinsics=(458.654, 457.296, 367.215, 248.375), distortion_model=0, distortion=(-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05))
CAM_EQUI = dict(width=512, height=512, intrinsics=(190.978, 190.973, 254.932, 256.897), distortion_model=1, distortion=(0.0034823894, 0.0007150348, -0.0020532361, 0.0002029367))
CAM_PLAIN = dict(width=640, height=480, intrinsics=(128.0, 128.0, 320.0, 240.0), distortion_model=0, distortion=(0.0, 0.0, 0.0, 0.0))
ALIGN = (np.cos(0.7), np.sin(0.7), (3.0, -2.0, 0.5))


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _to_map(p_c, R_wc, p_wc, align):
    p_w = p_c @ R_wc.T + p_wc
    if align is None:
        return p_w
    c, s, t = align
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return (p_w - np.asarray(t)) @ Rz


def too_close(j, cam, o):
    """points of a judge's answer that lie inside a margin of a threshold"""
    w, h = cam["width"], cam["height"]
    px, py, z, r2 = (np.asarray(j[k], np.float64) for k in ("px", "py", "depth", "r2"))
    with np.errstate(all="ignore"):
        bad = np.abs(z - o["min_depth"]) < DEPTH_MARGIN
        if np.isfinite(o["max_depth"]):
            bad |= np.abs(z - o["max_depth"]) < DEPTH_MARGIN
        if np.isfinite(o["max_r2"]):
            bad |= np.abs(r2 - o["max_r2"]) < DEPTH_MARGIN
        front = z > o["min_depth"]
        for v, size, cells in ((px, w, o["cols"]), (py, h, o["rows"])):
            edges = [o["margin"], size - 1 - o["margin"]] + [k * size / cells for k in range(1, cells)]
            for e in edges:
                bad |= front & (np.abs(v - e) < PIX_MARGIN)
    return bad


def random_case(n, cam, with_cov, with_cc, align, seed, **opt):
    """n points spread over and around the camera's view (about a fifth behind it, some far, some beside the image), in the map frame"""
    rng = np.random.default_rng([20261101, n, seed])
    o = R.options(**opt)
    R_wc = _rot(rng); p_wc = rng.uniform(-2, 2, 3)
    z = rng.uniform(-3.0, 12.0, n)
    half = 1.25 * np.array([cam["width"] / (2 * cam["intrinsics"][0]), cam["height"] / (2 * cam["intrinsics"][1])])
    p_c = np.concatenate([rng.uniform(-1, 1, (n, 2)) * half * z[:, None], z[:, None]], 1)
    cov = None
    if with_cov:
        A = rng.normal(size=(n, 3, 3))
        cov = 0.02 ** 2 * (A @ A.transpose(0, 2, 1) + 0.3 * np.eye(3))
    cc = None
    if with_cc:
        B = rng.normal(size=(6, 6)); D = np.diag([0.01, 0.01, 0.01, 0.03, 0.03, 0.03])
        cc = D @ (B @ B.T / 6 + 0.3 * np.eye(6)) @ D
    X = _to_map(p_c, R_wc, p_wc, align)
    bad = too_close(R.judge(X, cov, cam, align, R_wc, p_wc, cc, o), cam, o)
    if bad.any():
        X[bad] = _to_map(np.tile([[0.0, 0.0, -5.0]], (int(bad.sum()), 1)), R_wc, p_wc, align)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return dict(X=X, cov=cov, desc=desc, cam=cam, align=align, R_wc=R_wc, p_wc=p_wc, cov_cam=cc, opt=opt, o=o, exact=False)


def _plain_case(p_c, cov=None, exact=False, want=None, **opt):
    """identity pose and alignment, no distortion, integer intrinsics: the map frame is the camera frame"""
    p_c = np.asarray(p_c, np.float64).reshape(-1, 3)
    rng = np.random.default_rng(len(p_c))
    return dict(X=p_c, cov=cov, desc=rng.integers(0, 256, (len(p_c), 32), dtype=np.uint8), cam=CAM_PLAIN, align=None, R_wc=np.eye(3), p_wc=np.zeros(3), cov_cam=None, opt=opt,
                o=R.options(**opt), exact=exact, want=want or {})


def _pixel_points(px, py, z=2.0):
    """camera-frame points that land on the pixels (px, py) of CAM_PLAIN at depth z (exact for z a power of two and px, py on the 1/64 grid)"""
    px = np.asarray(px, np.float64); py = np.broadcast_to(np.asarray(py, np.float64), px.shape)
    return np.stack([(px - 320.0) / 128.0 * z, (py - 240.0) / 128.0 * z, np.full(px.shape, z)], -1)


def _hand_cases():
    c = {}
    behind = np.array([0.0, 0.0, -1.0])
    # all in one cell with quota 3 over four chunks; the first visible points are 300, 600 and 900, a fourth at 950 is one too many
    P = np.tile(behind, (1000, 1)); P[[300, 600, 900, 950]] = _pixel_points([100.5, 200.25, 300.0, 400.0], 100.0)
    c["one_cell_quota3_four_chunks"] = _plain_case(P, rows=1, cols=1, quota=3, want=dict(index=[300, 600, 900]))
    # the first three chunks hold nothing visible
    P = np.tile(behind, (1000, 1)); P[768:] = _pixel_points(np.linspace(20.5, 600.5, 232), np.linspace(30.25, 400.25, 232))
    c["visible_only_in_last_chunk"] = _plain_case(P, rows=2, cols=2, quota=100)
    # 1 x 2 cells, quota 5: five points in the left cell (exactly the quota), six in the right one (one over: index 10 is dropped)
    c["cell_at_quota_and_one_over"] = _plain_case(_pixel_points([10.5, 500.5, 20.5, 510.5, 30.5, 520.5, 40.5, 530.5, 50.5, 540.5, 550.5], 200.0), rows=1, cols=2, quota=5,
                                                  want=dict(index=[0, 2, 4, 6, 8, 1, 3, 5, 7, 9]))
    c["all_behind"] = _plain_case(np.tile(behind, (300, 1)) * np.arange(1, 301)[:, None], want=dict(index=[]))
    # exact edges, margin 8, min_depth 0.5: px = 8 and 631 inclusive, 7.984375 and 631.015625 outside; z == min_depth is BEHIND; a NaN or an
    # infinity in x or y reaches p_c,z through 0 x inf = NaN and is BEHIND, a NaN depth too, an infinite depth is FAR; a negative definite
    # covariance gives r_max
    P = np.concatenate([_pixel_points([8.0, 631.0, 7.984375, 631.015625, 320.0, 320.0], [100.0, 100.0, 100.0, 100.0, 8.0, 471.0]), _pixel_points([320.0], [240.0], 0.5),
                        [[np.nan, 0.0, 2.0], [0.0, 0.0, np.nan], [np.inf, 0.0, 2.0], [0.0, 0.0, np.inf], [0.25, 0.25, 2.0]]])
    cov = np.tile(1e-4 * np.eye(3), (len(P), 1, 1)); cov[-1] = -np.eye(3)
    c["exact_edges"] = _plain_case(P, cov=cov, exact=True, margin=8.0, min_depth=0.5, max_depth=100.0,
                                   want=dict(status=[R.VISIBLE, R.VISIBLE, R.OUTSIDE, R.OUTSIDE, R.VISIBLE, R.VISIBLE, R.BEHIND, R.BEHIND, R.BEHIND, R.BEHIND, R.FAR, R.VISIBLE],
                                             index=[0, 4, 1, 11, 5], last_radius=40.0))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    A = ALIGN
    c = {
        "n0_radtan": random_case(0, CAM_RADTAN, False, False, None, 0),
        "n1_radtan_cov": random_case(1, CAM_RADTAN, True, False, None, 1),
        "n63_equi": random_case(63, CAM_EQUI, False, False, None, 2),
        "n64_radtan_cov_cc_align": random_case(64, CAM_RADTAN, True, True, A, 3),
        "n65_equi_cov": random_case(65, CAM_EQUI, True, False, None, 4),
        "n257_radtan_cc": random_case(257, CAM_RADTAN, False, True, None, 5),
        "n5000_radtan_cov_cc_align": random_case(5000, CAM_RADTAN, True, True, A, 6),
        "n5000_equi_cov_cc_align_opts": random_case(5000, CAM_EQUI, True, True, A, 7, max_depth=8.0, margin=5.0, rows=3, cols=7, quota=10, k_sigma=2.0, sigma_px=1.5, r_min=2.0,
                                                    r_max=60.0, max_r2=1.2),
        "n5000_radtan_grid16": random_case(5000, CAM_RADTAN, True, False, A, 8, rows=16, cols=16, quota=4),
        "n70000_radtan_cov_cc_align": random_case(70000, CAM_RADTAN, True, True, A, 9),
    }
    c.update(_hand_cases())
    for v in c.values():
        v.setdefault("want", {})
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's answer, computed once per session and shared (read-only)"""
    k = cases()[name]
    return R.run(k["X"], k["cov"], k["desc"], k["cam"], k["align"], k["R_wc"], k["p_wc"], k["cov_cam"], k["o"])


@functools.lru_cache(maxsize=None)
def judged(name):
    k = cases()[name]
    return R.judge(k["X"], k["cov"], k["cam"], k["align"], k["R_wc"], k["p_wc"], k["cov_cam"], k["o"])
