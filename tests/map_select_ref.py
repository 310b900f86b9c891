"""CPU restatements of lvk_map_select_queries (include/lvk_c.h states the contract), for the tests only:

project     numpy float64, every expression in the header's order (numpy evaluates an expression as written, without contraction): status,
            cell, pixel, radius and depth of every point
select      the header's selection rule, vectorised (a stable sort by cell, a rank inside the cell)
select_loop the same rule as a plain Python double loop over cells and points - what `select` is held to
judge       pixel and radius in long double (x87 80-bit where numpy has it): what the float32 outputs are held to
run         project + select -> the arrays the GPU entry writes (MAP_SEL, MATCH_QUERY, descriptors, MAP_INFO, status bytes)"""
import numpy as np

from larvio_amd._lib import MAP_SEL, MAP_INFO, MATCH_QUERY

LD = np.longdouble
VISIBLE, BEHIND, FAR, OUTSIDE = 0, 1, 2, 3
SELECTED = 0x80
DEFAULTS = dict(min_depth=0.1, max_depth=np.inf, max_r2=np.inf, margin=0.0, k_sigma=3.0, sigma_px=1.0, r_min=4.0, r_max=40.0, rows=4, cols=5, quota=0)


def options(**kw):
    """the options with the header's defaults filled in (a zero field takes its default)"""
    o = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in o, k
        if v != 0:
            o[k] = v
    if o["quota"] == 0:
        o["quota"] = 1024 // (o["rows"] * o["cols"])
    return o


def _distort(x, y, r2, model, dist, T):
    one, two = T(1.0), T(2.0)
    if model == 0:
        k1, k2, p1, p2 = (T(v) for v in dist)
        rad = one + (k2 * r2 + k1) * r2
        xd = x * rad + two * p1 * x * y + p2 * (r2 + two * x * x)
        yd = y * rad + p1 * (r2 + two * y * y) + two * p2 * x * y
        return xd, yd
    d = [T(v) for v in dist]
    r = np.sqrt(r2)
    th = np.arctan(r); t2 = th * th
    thd = th * (one + t2 * (d[0] + t2 * (d[1] + t2 * (d[2] + t2 * d[3]))))
    with np.errstate(all="ignore"):
        s = np.where(r > T(1e-8), thd / r, one)
    return x * s, y * s


def _chain(X, cov, cam, align, R_wc, p_wc, cov_cam, o, T):
    """pose, model and radius in the arithmetic T (np.float64: the header's order exactly; np.longdouble: the judge)"""
    X = np.asarray(X, np.float64).reshape(-1, 3).astype(T)
    n = len(X)
    c, s, t = (T(1.0), T(0.0), np.zeros(3, T)) if align is None else (T(align[0]), T(align[1]), np.asarray(align[2], np.float64).astype(T))
    Rw = np.asarray(R_wc, np.float64).reshape(3, 3).astype(T); p = np.asarray(p_wc, np.float64).reshape(3).astype(T)
    fx, fy, cx, cy = (T(v) for v in cam["intrinsics"])
    with np.errstate(all="ignore"):
        q0 = c * X[:, 0] - s * X[:, 1]; q1 = s * X[:, 0] + c * X[:, 1]
        g = [(q0 + t[0]) - p[0], (q1 + t[1]) - p[1], (X[:, 2] + t[2]) - p[2]]
        pc = [(Rw[0, i] * g[0] + Rw[1, i] * g[1]) + Rw[2, i] * g[2] for i in range(3)]
        x = pc[0] / pc[2]; y = pc[1] / pc[2]
        r2 = x * x + y * y
        xd, yd = _distort(x, y, r2, cam["distortion_model"], cam["distortion"], T)
        px = fx * xd + cx; py = fy * yd + cy
        lam = np.zeros(n, T)
        if cov is not None or cov_cam is not None:
            S = None
            if cov is not None:
                Sx = np.asarray(cov, np.float64).reshape(-1, 3, 3).astype(T)
                R = np.empty((3, 3), T)
                for j in range(3):
                    R[0, j] = c * Rw[0, j] + s * Rw[1, j]; R[1, j] = c * Rw[1, j] - s * Rw[0, j]; R[2, j] = Rw[2, j]
                M = [[(Sx[:, i, 0] * R[0, j] + Sx[:, i, 1] * R[1, j]) + Sx[:, i, 2] * R[2, j] for j in range(3)] for i in range(3)]
                S = [[(R[0, i] * M[0][j] + R[1, i] * M[1][j]) + R[2, i] * M[2][j] for j in range(3)] for i in range(3)]
            if cov_cam is not None:
                C = np.asarray(cov_cam, np.float64).reshape(6, 6).astype(T)
                z = np.zeros(n, T); full = lambda v: np.full(n, v, T)
                G = [[z, -pc[2], pc[1], full(-Rw[0, 0]), full(-Rw[1, 0]), full(-Rw[2, 0])],
                     [pc[2], z, -pc[0], full(-Rw[0, 1]), full(-Rw[1, 1]), full(-Rw[2, 1])],
                     [-pc[1], pc[0], z, full(-Rw[0, 2]), full(-Rw[1, 2]), full(-Rw[2, 2])]]
                Tm = [[None] * 6 for _ in range(3)]
                for i in range(3):
                    for k in range(6):
                        acc = G[i][0] * C[0, k]
                        for m in range(1, 6):
                            acc = acc + G[i][m] * C[m, k]
                        Tm[i][k] = acc
                K = [[None] * 3 for _ in range(3)]
                for i in range(3):
                    for j in range(3):
                        acc = Tm[i][0] * G[j][0]
                        for k in range(1, 6):
                            acc = acc + Tm[i][k] * G[j][k]
                        K[i][j] = acc
                S = K if S is None else [[S[i][j] + K[i][j] for j in range(3)] for i in range(3)]
            u = [S[0][j] - x * S[2][j] for j in range(3)]; v = [S[1][j] - y * S[2][j] for j in range(3)]
            e00 = u[0] - u[2] * x; e01 = u[1] - u[2] * y; e10 = v[0] - v[2] * x; e11 = v[1] - v[2] * y
            sx = fx / pc[2]; sy = fy / pc[2]
            a = (sx * sx) * e00; d = (sy * sy) * e11; b = ((sx * sy) * e01 + (sx * sy) * e10) / T(2.0)
            hd = (a - d) / T(2.0)
            lam = (a + d) / T(2.0) + np.sqrt(hd * hd + b * b)
        sig = T(o["sigma_px"])
        rad = T(o["k_sigma"]) * np.sqrt(lam + sig * sig)
        rad = np.where(rad < T(o["r_min"]), T(o["r_min"]), np.where(rad > T(o["r_max"]), T(o["r_max"]), rad))
        rad = np.where((lam >= 0) & np.isfinite(lam), rad, T(o["r_max"]))
    return dict(pc=pc, x=x, y=y, r2=r2, px=px, py=py, radius=rad, lam=lam)


def project(X, cov, cam, align, R_wc, p_wc, cov_cam, o, T=np.float64):
    """-> dict(status (n,) uint8, cell (n,) int32 (0 where not VISIBLE), px, py, radius, depth in T, r2)"""
    k = _chain(X, cov, cam, align, R_wc, p_wc, cov_cam, o, T)
    w, h = cam["width"], cam["height"]
    z, px, py = k["pc"][2], k["px"], k["py"]
    m = T(o["margin"]); hx = T(w - 1) - m; hy = T(h - 1) - m
    with np.errstate(all="ignore"):
        behind = ~(z > T(o["min_depth"]))
        far = z > T(o["max_depth"])
        out1 = ~(k["r2"] <= T(o["max_r2"]))
        out2 = ~((m <= px) & (px <= hx) & (m <= py) & (py <= hy))
        status = np.where(behind, BEHIND, np.where(far, FAR, np.where(out1 | out2, OUTSIDE, VISIBLE))).astype(np.uint8)
        vis = status == VISIBLE
        col = np.where(vis, (px * T(o["cols"])) / T(w), 0).astype(np.int64); row = np.where(vis, (py * T(o["rows"])) / T(h), 0).astype(np.int64)
    cell = np.where(vis, np.minimum(o["rows"] - 1, row) * o["cols"] + np.minimum(o["cols"] - 1, col), 0).astype(np.int32)
    return dict(status=status, cell=cell, px=px, py=py, radius=k["radius"], depth=z, r2=k["r2"], lam=k["lam"])


def select(status, cell, n_cells, quota):
    """the selected map indices in output order: every cell's `quota` lowest VISIBLE indices, by (cell, index)"""
    idx = np.nonzero(status == VISIBLE)[0]
    order = np.argsort(cell[idx], kind="stable")
    idx = idx[order]; c = cell[idx]
    first = np.searchsorted(c, np.arange(n_cells))
    rank = np.arange(len(idx)) - first[c]
    return idx[rank < quota]


def select_loop(status, cell, n_cells, quota):
    out = []
    for c in range(n_cells):
        kept = 0
        for i in range(len(status)):
            if status[i] == VISIBLE and cell[i] == c and kept < quota:
                out.append(i); kept += 1
    return np.array(out, np.int64)


def run(X, cov, desc, cam, align, R_wc, p_wc, cov_cam, o):
    """what the GPU entry writes: dict(info, sel, q, q_desc, status, proj)"""
    pr = project(X, cov, cam, align, R_wc, p_wc, cov_cam, o)
    idx = select(pr["status"], pr["cell"], o["rows"] * o["cols"], o["quota"])
    sel = np.zeros(len(idx), MAP_SEL)
    sel["index"] = idx; sel["cell"] = pr["cell"][idx]
    sel["x"] = pr["px"][idx].astype(np.float32); sel["y"] = pr["py"][idx].astype(np.float32)
    sel["radius"] = pr["radius"][idx].astype(np.float32); sel["depth"] = pr["depth"][idx].astype(np.float32)
    q = np.zeros(len(idx), MATCH_QUERY)
    q["x"], q["y"], q["radius"] = sel["x"], sel["y"], sel["radius"]
    info = np.zeros(1, MAP_INFO)[0]
    info["n_selected"] = len(idx)
    for f, s in (("n_visible", VISIBLE), ("n_behind", BEHIND), ("n_far", FAR), ("n_outside", OUTSIDE)):
        info[f] = int((pr["status"] == s).sum())
    status = pr["status"].copy(); status[idx] |= SELECTED
    return dict(info=info, sel=sel, q=q, q_desc=None if desc is None else np.asarray(desc, np.uint8).reshape(-1, 32)[idx], status=status, proj=pr)


def judge(X, cov, cam, align, R_wc, p_wc, cov_cam, o):
    """pixel and radius of every point in long double, rounded to float32 once: dict(x, y, radius as float32; px, py, depth, r2 as LD)"""
    pr = project(X, cov, cam, align, R_wc, p_wc, cov_cam, o, T=LD)
    with np.errstate(all="ignore"):
        return dict(x=pr["px"].astype(np.float32), y=pr["py"].astype(np.float32), radius=pr["radius"].astype(np.float32), px=pr["px"], py=pr["py"], depth=pr["depth"],
                    r2=pr["r2"], status=pr["status"], cell=pr["cell"], lam=pr["lam"])


def adjacent_or_equal(a, b):
    """float32 arrays: equal, or neighbours in the float32 number line"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return (a == b) | (np.nextafter(a, b) == b)
