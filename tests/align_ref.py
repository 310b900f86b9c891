"""Restatement of what lvk_align_ransac_2pt and lvk_align_draw_pairs (include/lvk_c.h) define, written from the geometry: both frames have
z along gravity, p_w = Rz(psi) X + t is sought; a pair of matches fixes it through Rz (X_i - X_j) = l_i d_i - l_j d_j, whose z row is linear
in the two depths and whose xy norm is then one quadratic.

One body of code runs in three arithmetics (`kind`):
  "ld"   np.longdouble - the judge;
  "f64"  np.float64, the same expressions in the same order - the evidence that the margins below are enough for FP64;
  "v"    class V of tests/msckf_point_ref.py: the long-double value with a first-order running bound on the error of its float64
         evaluation, operation by operation (sqrt: e / (2 sqrt) + u sqrt, so the 1 / sqrt(disc) and 1 / d_z terms of the solver are carried).
run() returns every discrete result (n_models, counts, winner, mask, status, iterations), the continuous ones, and the margins that make
the discrete ones well defined: per case the smallest relative distance of any squared residual from thresh^2, of any camera depth from
min_depth, of either solved depth from 0 (relative to the terms it is the sum of), of the discriminant from 0 (relative to B^2), of the
divisor |d_z| from min_dz, of the two |d_z| from each other (which bearing divides), of a refinement step from the stop rule, of a Cholesky
pivot from its threshold - and whether two models tie for the best count.

bounds() gives the GPU tests their tolerances: for every model of the solver the V-carried error, doubled; for the refined model
|A^-1| times the V-carried error of the gradient sum at the final iterate (the refinement ends at a stationary point of the float64
gradient: what moves it is the rounding of that gradient, seen through the inverse of the normal matrix) plus three roundings of the
update itself, doubled; for A and the rms their V evaluation with the model carrying that bound, doubled.  Every constant is a count of
operations."""
import numpy as np

from tests.msckf_point_ref import V, LD, U, U_LD

OK, NO_MODEL, FEW_INLIERS, SINGULAR = 0, 1, 2, 3
DEFAULT_SEED = 0xFFFFFFFF
MAX_PAIRS = 4096
STEP_TOL2 = 1e-20
PIVOT_REL = 1e-12
DEFAULTS = dict(thresh=0.01, min_depth=0.1, min_dz=1e-6, min_inliers=6, max_refine_iters=10)
# why a pair gave no model
R_MODEL, R_INDEX, R_BASELINE, R_MIN_DZ, R_LEADING, R_DISC, R_DEPTHS = 0, 1, 2, 3, 4, 5, 6


# ------------------------------------------------------------------------------------------------ arithmetic kinds
def _conv(a, kind):
    a = np.asarray(a, np.float64)
    return a.copy() if kind == "f64" else a.astype(LD) if kind == "ld" else V(a.astype(LD))


def _v(x):
    return x.v if isinstance(x, V) else x


def _sqrt(x):
    if isinstance(x, V):
        r = np.sqrt(x.v)
        return V(r, x.e / (2 * r) + U * r)
    return np.sqrt(x)


def _where(c, a, b):
    if isinstance(a, V) or isinstance(b, V):
        a = a if isinstance(a, V) else V(a); b = b if isinstance(b, V) else V(b)
        return V(np.where(c, a.v, b.v), np.where(c, a.e, b.e))
    return np.where(c, a, b)


def _sum(x):
    """a sum of n terms in any order: the terms' own errors and (n - 1) u sum |x|"""
    if isinstance(x, V):
        n = x.v.shape[0]
        return V(x.v.sum(0), x.e.sum(0) + max(n - 1, 0) * U * np.abs(x.v).sum(0))
    return x.sum(0)


def options(**kw):
    o = dict(DEFAULTS); o.update({k: v for k, v in kw.items() if v})
    return o


# ------------------------------------------------------------------------------------------------ the pair drawing
def draw_pairs(n, max_hypotheses=0, seed=0):
    """every pair i < j in lexicographic order when there are at most max_hypotheses (0: 4096) of them, otherwise max_hypotheses draws
    i = r() % n, j = r() % (n - 1), j += (j >= i) of the multiply-with-carry generator x <- low32(x) * 4164903690 + (x >> 32)"""
    mh = max_hypotheses or MAX_PAIRS
    if n < 2:
        return np.zeros((0, 2), np.int32)
    if n * (n - 1) // 2 <= mh:
        return np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32)
    state = seed or DEFAULT_SEED
    out = []

    def r():
        nonlocal state
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
        return state & 0xFFFFFFFF
    for _ in range(mh):
        i = r() % n; j = r() % (n - 1); j += j >= i
        out.append((i, j))
    return np.array(out, np.int32)


# ------------------------------------------------------------------------------------------------ the minimal solver
def solve(X, uv, pairs, R_wc, p_wc, min_dz, kind, mutate=None):
    """All pairs at once.  -> dict(valid (P, 2) bool by ROOT, c, s (P, 2), t (P, 2, 3) in `kind`, reason (P,), margins, flags)
    mutate: None, "sign_s" (s negated), "small_dz" (the bearing with the smaller |d_z| divides)"""
    n = len(X); pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    i, j = pairs[:, 0], pairs[:, 1]
    ok = (i != j) & (i >= 0) & (j >= 0) & (i < n) & (j < n)
    ii, jj = np.where(ok, i, 0), np.where(ok, j, 0)
    if n == 0:
        ii = jj = np.zeros(len(pairs), np.int64); X = np.zeros((1, 3)); uv = np.zeros((1, 2))
    Xk = _conv(X, kind); u = _conv(uv[:, 0], kind); v = _conv(uv[:, 1], kind)
    R = _conv(np.asarray(R_wc, np.float64).reshape(3, 3), kind); p = _conv(p_wc, kind)
    with np.errstate(all="ignore"):
        di = [(R[r, 0] * u[ii] + R[r, 1] * v[ii]) + R[r, 2] for r in range(3)]
        dj = [(R[r, 0] * u[jj] + R[r, 1] * v[jj]) + R[r, 2] for r in range(3)]
        Xi = [Xk[ii, k] for k in range(3)]
        a = [Xi[k] - Xk[jj, k] for k in range(3)]
        rho2 = a[0] * a[0] + a[1] * a[1]
        adi, adj = np.abs(_v(di[2])), np.abs(_v(dj[2]))
        pi = adi >= adj
        if mutate == "small_dz":
            pi = ~pi
        dzmax = np.where(pi, adi, adj)
        ok1 = ok & (_v(rho2) > 0)
        ok2 = ok1 & (dzmax >= min_dz)
        al_i = a[2] / di[2]; be_i = dj[2] / di[2]
        al_j = (-a[2]) / dj[2]; be_j = di[2] / dj[2]
        alpha = _where(pi, al_i, al_j); beta = _where(pi, be_i, be_j)
        e = [_where(pi, al_i * di[k], (-al_j) * dj[k]) for k in range(2)]
        f = [_where(pi, be_i * di[k] - dj[k], di[k] - be_j * dj[k]) for k in range(2)]
        A = f[0] * f[0] + f[1] * f[1]; B = e[0] * f[0] + e[1] * f[1]; C = (e[0] * e[0] + e[1] * e[1]) - rho2
        disc = B * B - A * C
        ok3 = ok2 & (_v(A) > 0)
        ok4 = ok3 & (_v(disc) >= 0)
        sq = _sqrt(_where(ok4, disc, _conv(np.ones(len(pairs)), kind)))
        valid = np.zeros((len(pairs), 2), bool); cs, ss, ts = [], [], []
        m_depth = np.inf; opposite = np.zeros(len(pairs), bool)
        for root in range(2):
            mu = ((-B) - sq if root == 0 else (-B) + sq) / A
            lp = alpha + beta * mu
            muv, lpv = _v(mu), _v(lp)
            valid[:, root] = ok4 & (muv > 0) & (lpv > 0)
            opposite |= ok4 & ((muv > 0) != (lpv > 0))
            if ok4.any():
                sc_mu = (np.abs(_v(B)) + _v(sq)) / _v(A); sc_lp = np.abs(_v(alpha)) + np.abs(_v(beta) * muv)
                m_depth = min(m_depth, float(np.min(np.abs(muv[ok4]) / sc_mu[ok4])), float(np.min(np.abs(lpv[ok4]) / sc_lp[ok4])))
            li = _where(pi, lp, mu)
            w0 = e[0] + mu * f[0]; w1 = e[1] + mu * f[1]
            dot = a[0] * w0 + a[1] * w1; crs = a[0] * w1 - a[1] * w0
            nrm = _sqrt(dot * dot + crs * crs)
            c = dot / nrm; s = crs / nrm
            if mutate == "sign_s":
                s = -s
            t = [(p[0] + li * di[0]) - (c * Xi[0] - s * Xi[1]), (p[1] + li * di[1]) - (s * Xi[0] + c * Xi[1]), (p[2] + li * di[2]) - Xi[2]]
            cs.append(c); ss.append(s); ts.append(t)
    reason = np.full(len(pairs), R_DEPTHS)
    reason[valid.any(1)] = R_MODEL
    for cond, code in ((ok3 & ~ok4, R_DISC), (ok2 & ~ok3, R_LEADING), (ok1 & ~ok2, R_MIN_DZ), (ok & ~ok1, R_BASELINE), (~ok, R_INDEX)):
        reason[cond] = code
    differ = ok1 & (adi != adj)
    margins = dict(
        depth0=m_depth,
        disc=float(np.min(np.abs(_v(disc)[ok3]) / (_v(B)[ok3] ** 2))) if ok3.any() else np.inf,
        min_dz=float(np.min(np.abs(dzmax[ok1] - min_dz) / min_dz)) if ok1.any() else np.inf,
        divisor=float(np.min(np.abs(adi[differ] - adj[differ]) / np.maximum(adi[differ], adj[differ]))) if differ.any() else np.inf)
    return dict(valid=valid, c=cs, s=ss, t=ts, reason=reason, margins=margins, opposite=opposite, two=valid.all(1), dz_zero=ok2 & (np.minimum(adi, adj) == 0))


# ------------------------------------------------------------------------------------------------ the score
def cam_points(c, s, t, Xk, R, p):
    """p_c = R_wc^T ((Rz X + t) - p_wc) in the kernel's order; c, s: (M, 1) or scalars, t: three of them; Xk: three (n,) arrays"""
    q0 = c * Xk[0] - s * Xk[1]; q1 = s * Xk[0] + c * Xk[1]
    g0 = (q0 + t[0]) - p[0]; g1 = (q1 + t[1]) - p[1]; g2 = (Xk[2] + t[2]) - p[2]
    x = (R[0, 0] * g0 + R[1, 0] * g1) + R[2, 0] * g2
    y = (R[0, 1] * g0 + R[1, 1] * g1) + R[2, 1] * g2
    z = (R[0, 2] * g0 + R[1, 2] * g1) + R[2, 2] * g2
    return q0, q1, x, y, z


def score(c, s, t, X, uv, R_wc, p_wc, thresh2, min_depth, kind, transpose_bug=False):
    """inlier flags (M, n) of M models (c, s (M,), t (M, 3) in `kind`) and the margins of the two tests"""
    Xk = [_conv(X[:, k], kind)[None, :] for k in range(3)]; u = _conv(uv[:, 0], kind)[None, :]; v = _conv(uv[:, 1], kind)[None, :]
    R = _conv(np.asarray(R_wc, np.float64).reshape(3, 3), kind); p = _conv(p_wc, kind)
    if transpose_bug:
        R = R.T
    th2 = _conv(thresh2, kind); md = _conv(min_depth, kind)
    inl = np.zeros((len(c), X.shape[0]), bool); m_res = m_z = np.inf
    for lo in range(0, len(c), 128):
        sl = slice(lo, lo + 128)
        with np.errstate(all="ignore"):
            _, _, x, y, z = cam_points(c[sl, None], s[sl, None], [t[sl, k, None] for k in range(3)], Xk, R, p)
            front = z > md
            rx = x / z - u; ry = y / z - v
            r2 = rx * rx + ry * ry
            inl[sl] = front & (r2 <= th2)
            if front.any():
                m_res = min(m_res, float(np.min(np.abs(r2[front] - th2) / th2)))
            if z.size:
                m_z = min(m_z, float(np.min(np.abs(z - md) / md)))
    return inl, dict(resid=m_res, cam_depth=m_z)


# ------------------------------------------------------------------------------------------------ the refinement
def gn_sums(c, s, t, X, uv, R_wc, p_wc, kind):
    """A (4 x 4), g (4), sum |r|^2 over the matches given, at (c, s, t) - scalars of `kind` (V: with what they carry)"""
    Xk = [_conv(X[:, k], kind) for k in range(3)]; u = _conv(uv[:, 0], kind); v = _conv(uv[:, 1], kind)
    R = _conv(np.asarray(R_wc, np.float64).reshape(3, 3), kind); p = _conv(p_wc, kind)
    q0, q1, x, y, z = cam_points(c, s, t, Xk, R, p)
    one = _conv(1.0, kind)
    iz = one / z; a = x * iz; b = y * iz
    rx = a - u; ry = b - v
    dx = [R[1, 0] * q0 - R[0, 0] * q1, R[0, 0], R[1, 0], R[2, 0]]
    dy = [R[1, 1] * q0 - R[0, 1] * q1, R[0, 1], R[1, 1], R[2, 1]]
    dz = [R[1, 2] * q0 - R[0, 2] * q1, R[0, 2], R[1, 2], R[2, 2]]
    jx = [(dx[k] - a * dz[k]) * iz for k in range(4)]; jy = [(dy[k] - b * dz[k]) * iz for k in range(4)]
    A = [[None] * 4 for _ in range(4)]
    for k in range(4):
        for r in range(k, 4):
            A[k][r] = A[r][k] = _sum(jx[k] * jx[r] + jy[k] * jy[r])
    g = [_sum(jx[k] * rx + jy[k] * ry) for k in range(4)]
    # sum |J^T| |r|, the scale of the gradient, and its floor: a residual is known no better than the ~16 roundings of this file's
    # arithmetic behind it (an exactly solvable problem has r = 0 and a gradient of rounding alone)
    absg = np.array([float(np.sum(np.abs(_v(jx[k]) * _v(rx)) + np.abs(_v(jy[k]) * _v(ry)))) for k in range(4)])
    fx = 16 * U_LD * (np.abs(_v(a)) + np.abs(_v(u))); fy = 16 * U_LD * (np.abs(_v(b)) + np.abs(_v(v)))
    floor = np.array([float(np.sum(np.abs(_v(jx[k])) * fx + np.abs(_v(jy[k])) * fy)) for k in range(4)])
    return A, g, _sum(rx * rx + ry * ry), (absg, floor)


def chol_solve(A, g):
    """A d = -g by the kernel's Cholesky, its pivot rule included -> (d or None, smallest pivot / (PIVOT_REL * diagonal) - 1)"""
    a00, a01, a02, a03, a11, a12, a13, a22, a23, a33 = A[0][0], A[0][1], A[0][2], A[0][3], A[1][1], A[1][2], A[1][3], A[2][2], A[2][3], A[3][3]
    with np.errstate(all="ignore"):
        l00 = np.sqrt(a00); l10 = a01 / l00; l20 = a02 / l00; l30 = a03 / l00
        p1 = a11 - l10 * l10
        l11 = np.sqrt(p1); l21 = (a12 - l20 * l10) / l11; l31 = (a13 - l30 * l10) / l11
        p2 = (a22 - l20 * l20) - l21 * l21
        l22 = np.sqrt(p2); l32 = ((a23 - l30 * l20) - l31 * l21) / l22
        p3 = ((a33 - l30 * l30) - l31 * l31) - l32 * l32
        pd = a00 > 0
        margin = np.inf
        for piv, diag in ((p1, a11), (p2, a22), (p3, a33)):
            if pd:
                pd = bool(piv > PIVOT_REL * diag)
                margin = min(margin, abs(float(piv / (PIVOT_REL * diag)) - 1.0)) if diag > 0 else 0.0
        if not pd:
            return None, margin
        l33 = np.sqrt(p3)
        y0 = -g[0] / l00; y1 = (-g[1] - l10 * y0) / l11; y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22; y3 = (((-g[3] - l30 * y0) - l31 * y1) - l32 * y2) / l33
        d3 = y3 / l33; d2 = (y2 - l32 * d3) / l22; d1 = ((y1 - l21 * d2) - l31 * d3) / l11; d0 = (((y0 - l10 * d1) - l20 * d2) - l30 * d3) / l00
    return [d0, d1, d2, d3], margin


def refine(c, s, t, X, uv, R_wc, p_wc, max_iters, kind):
    """Gauss-Newton from (c, s, t) over the matches given, to the header's stop rule.
    -> dict(status, c, s, t, A, rms, iters, margins(step, pivot), grad, absg)"""
    t = list(t); iters = 0; status = OK; last = False
    c0, s0, t0 = c, s, list(t)
    m_step = m_piv = np.inf
    half = _conv(0.5, kind); one = _conv(1.0, kind)
    while True:
        A, g, ssq, absg = gn_sums(c, s, t, X, uv, R_wc, p_wc, kind)
        if last or iters >= max_iters:
            break
        d, mp = chol_solve(A, g)
        m_piv = min(m_piv, mp)
        if d is None:
            status = SINGULAR
            break
        hh = half * d[0]; h2 = hh * hh; den = one + h2; cd = (one - h2) / den; sd = (hh + hh) / den
        c, s = c * cd - s * sd, s * cd + c * sd
        t = [t[0] + d[1], t[1] + d[2], t[2] + d[3]]
        iters += 1
        step2 = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]
        last = bool(step2 <= STEP_TOL2)
        m_step = min(m_step, abs(float(step2) / STEP_TOL2 - 1.0))
    if status != OK:
        c, s, t = c0, s0, t0
    return dict(status=status, c=c, s=s, t=t, A=np.array(A), rms=np.sqrt(ssq / _conv(float(len(X)), kind)), iters=iters, grad=np.array(g), absg=absg[0], gfloor=absg[1],
                margins=dict(step=m_step, pivot=m_piv))


# ------------------------------------------------------------------------------------------------ the whole call
def run(X, uv, pairs, R_wc, p_wc, opt=None, kind="ld", mutate=None):
    """lvk_align_ransac_2pt on n = len(X) matches and the pairs given.  -> dict: n_models (P,), count (P, 2) by SLOT (-1: no model), root
    (P, 2) by slot, c, s (P, 2), t (P, 2, 3) by slot, reason, status, hyp, slot, root_w, n_inliers, mask, the minimal and the refined model,
    A, rms, iters, margins, tie (two models share the best count), flags.  mutate: see solve(); "transpose" (R_wc for R_wc^T in the score);
    "tie_high" (ties to the highest index)"""
    assert kind in ("ld", "f64")
    o = options(**(opt or {}))
    X = np.asarray(X, np.float64).reshape(-1, 3); uv = np.asarray(uv, np.float64).reshape(-1, 2)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n, P = len(X), len(pairs)
    dt = np.float64 if kind == "f64" else LD
    out = dict(n_models=np.zeros(P, np.int32), count=np.full((P, 2), -1, np.int64), root=np.full((P, 2), -1, np.int32), c=np.zeros((P, 2), dt), s=np.zeros((P, 2), dt),
               t=np.zeros((P, 2, 3), dt), reason=np.full(P, R_INDEX), mask=np.zeros(n, np.uint8), status=NO_MODEL, hyp=-1, slot=-1, root_w=-1, n_inliers=0, iters=0,
               tie=False, margins={}, min_model=(dt(1), dt(0), np.zeros(3, dt)), model=(dt(1), dt(0), np.zeros(3, dt)), A=np.zeros((4, 4), dt), rms=dt(0))
    if n < 2 or P == 0:
        return out
    thresh2 = np.float64(o["thresh"]) * np.float64(o["thresh"])
    sv = solve(X, uv, pairs, R_wc, p_wc, o["min_dz"], kind, mutate if mutate in ("sign_s", "small_dz") else None)
    out["reason"] = sv["reason"]; out["flags"] = dict(opposite=sv["opposite"], two=sv["two"], dz_zero=sv["dz_zero"])
    margins = dict(sv["margins"])
    valid = sv["valid"]
    hs, rs = np.nonzero(valid)                       # row-major: hypothesis, then root - the slot order
    if len(hs):
        c = np.array([sv["c"][r][h] for h, r in zip(hs, rs)], dt); s = np.array([sv["s"][r][h] for h, r in zip(hs, rs)], dt)
        t = np.array([[sv["t"][r][k][h] for k in range(3)] for h, r in zip(hs, rs)], dt)
        inl, ms = score(c, s, t, X, uv, R_wc, p_wc, thresh2, o["min_depth"], kind, transpose_bug=mutate == "transpose")
        margins.update(ms)
        cnt = inl.sum(1)
        slot = np.zeros(len(hs), int); slot[1:] = (hs[1:] == hs[:-1])
        out["n_models"] = np.bincount(hs, minlength=P).astype(np.int32)
        out["count"][hs, slot] = cnt; out["root"][hs, slot] = rs; out["c"][hs, slot] = c; out["s"][hs, slot] = s; out["t"][hs, slot] = t
        best = int(cnt.max())
        w = int(np.argmax(cnt)) if mutate != "tie_high" else int(len(cnt) - 1 - np.argmax(cnt[::-1]))
        out.update(tie=bool((cnt == best).sum() > 1), hyp=int(hs[w]), slot=int(slot[w]), root_w=int(rs[w]), n_inliers=best, mask=inl[w].astype(np.uint8),
                   min_model=(c[w], s[w], t[w].copy()), model=(c[w], s[w], t[w].copy()))
        if best < o["min_inliers"]:
            out["status"] = FEW_INLIERS
        else:
            sel = inl[w]
            rf = refine(c[w], s[w], t[w], X[sel], uv[sel], R_wc, p_wc, o["max_refine_iters"], kind)
            margins.update(rf["margins"])
            out.update(status=rf["status"], model=(rf["c"], rf["s"], np.array(rf["t"], dt)), A=rf["A"], rms=rf["rms"], iters=rf["iters"], grad=rf["grad"], absg=rf["absg"], gfloor=rf["gfloor"])
    out["margins"] = margins
    return out


DISCRETE = ("n_models", "count", "root", "reason", "mask", "status", "hyp", "slot", "root_w", "n_inliers", "iters")


def same_discrete(a, b):
    """the names of the discrete results in which two runs differ"""
    return [k for k in DISCRETE if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


# ------------------------------------------------------------------------------------------------ the bounds
def bounds(X, uv, pairs, R_wc, p_wc, ref, opt=None):
    """The tolerances of the GPU comparison against `ref` = run(.., kind="ld").  -> dict(c, s (P, 2), t (P, 2, 3) by slot; model (5,): c, s,
    t of the refined model; A (4, 4); rms)"""
    o = options(**(opt or {}))
    X = np.asarray(X, np.float64).reshape(-1, 3); uv = np.asarray(uv, np.float64).reshape(-1, 2)
    P = len(ref["n_models"])
    out = dict(c=np.zeros((P, 2), LD), s=np.zeros((P, 2), LD), t=np.zeros((P, 2, 3), LD), model=np.zeros(5, LD), A=np.zeros((4, 4), LD), rms=LD(0))
    if ref["status"] == NO_MODEL:
        return out
    extra = 1 + U_LD / U                                    # this file's own rounding of the same expressions
    sv = solve(X, uv, pairs, R_wc, p_wc, o["min_dz"], "v")
    for h in range(P):
        for slot in range(int(ref["n_models"][h])):
            r = int(ref["root"][h, slot])
            out["c"][h, slot] = 2 * extra * sv["c"][r].e[h]; out["s"][h, slot] = 2 * extra * sv["s"][r].e[h]
            out["t"][h, slot] = [2 * extra * sv["t"][r][k].e[h] for k in range(3)]
    w, ws = ref["hyp"], ref["slot"]
    e_min = np.array([out["c"][w, ws], out["s"][w, ws], *out["t"][w, ws]], LD)
    out["model"] = e_min.copy()
    if ref["status"] == FEW_INLIERS:
        return out
    sel = ref["mask"].astype(bool)
    c, s, t = ref["model"]
    if ref["status"] == OK:
        # the stationarity defect of the float64 gradient, through A^-1: (dpsi, dt), then dc = |s| dpsi, ds = |c| dpsi; three roundings
        # of the update on top (one product pair and one difference for c and s, one sum for t)
        _, g, _, _ = gn_sums(V(c), V(s), [V(x) for x in t], X[sel], uv[sel], R_wc, p_wc, "v")
        ge = np.array([x.e for x in g], LD)
        d = np.abs(np.linalg.inv(ref["A"].astype(np.float64))).astype(LD) @ ge
        e_x = np.array([abs(s) * d[0], abs(c) * d[0], d[1], d[2], d[3]], LD) + 3 * U * np.abs(np.array([c, s, *t], LD))
        out["model"] = 2 * extra * e_x
    em = out["model"]
    A, _, ssq, _ = gn_sums(V(c, em[0]), V(s, em[1]), [V(t[k], em[2 + k]) for k in range(3)], X[sel], uv[sel], R_wc, p_wc, "v")
    out["A"] = 2 * extra * np.array([[A[k][r].e for r in range(4)] for k in range(4)], LD)
    rms = _sqrt(ssq / V(LD(int(sel.sum()))))
    out["rms"] = 2 * extra * rms.e
    return out
