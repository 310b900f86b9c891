"""Restatement of what lvk_align_ransac_3d (include/lvk_c.h) defines: the yaw and translation Y = Rz(psi) X + t between two sessions'
frames, both with z along gravity, from putative 3D-3D matches.  A pair of matches fixes the yaw through the horizontal parts of
a = X_i - X_j and b = Y_i - Y_j (c = a.b / |a||b|, s = a x b / |a||b|) and the translation as the mean of the two residuals; the refinement
is the closed-form planar Procrustes over the winner's inliers.

One body of code runs in three arithmetics (`kind`), as tests/align_ref.py does:
  "ld"   np.longdouble - the judge;
  "f64"  np.float64, the same expressions in the same order - what the GPU's hypotheses, counts, winner and mask must equal bit for bit;
  "v"    class V of tests/msckf_point_ref.py: the long-double value with a first-order running bound on the error of its float64 evaluation.
decisions() runs the "v" kind over every comparison that decides something discrete - the solver's four (ra2 and rb2 against min_rho^2,
|a_z - b_z| and |sqrt ra2 - sqrt rb2| against 2 thresh), the inlier test of every model on every match, and the refinement's SINGULAR test -
and counts those whose two sides are closer than the bound the left side carries.  The arg-max compares integers: it is decided as soon as
no inlier test is flagged.  A comparison whose bound is exactly 0 (its operands came out exact) cannot be flagged: it has one answer in any
arithmetic.
bounds() gives the GPU tests their tolerances for the refined c, s, t, A and rms: the V-carried error of the closed form with its sums
taken in any order ((m - 1) u sum |x| per sum), doubled, times the rounding of this file's own arithmetic."""
import numpy as np

from tests.align_ref import _conv, _v, _sqrt, _sum, draw_pairs, OK, NO_MODEL, FEW_INLIERS, SINGULAR            # noqa: F401  (re-exported)
from tests.msckf_point_ref import V, LD, U, U_LD

DEFAULTS = dict(thresh=0.10, min_rho=0.5, min_inliers=6)
SING_REL = 1e-12
# why a pair gave no model
R_MODEL, R_INDEX, R_RHO, R_DZ, R_LENGTH = 0, 1, 2, 3, 4


def options(**kw):
    o = dict(DEFAULTS); o.update({k: v for k, v in kw.items() if v})
    return o


def _consts(o):
    """the three constants as the library's host code forms them, in float64"""
    th = np.float64(o["thresh"]); rho = np.float64(o["min_rho"])
    return th * th, 2.0 * th, rho * rho


def _abs(x):
    return V(np.abs(x.v), x.e) if isinstance(x, V) else np.abs(x)


def _near(lhs, rhs, where):
    """how many of the comparisons lhs <> rhs (where `where`) lie inside the bound lhs carries"""
    if not isinstance(lhs, V):
        return 0
    with np.errstate(all="ignore"):
        d = np.abs(lhs.v - LD(rhs))
        return int(np.sum(where & (lhs.e > 0) & (d <= 2 * lhs.e)))


def solve(X, Y, pairs, o, kind):
    """All pairs at once.  -> dict(valid (P,), c, s (P,), t: three (P,) in `kind`, reason (P,), flagged: comparisons inside their bound)"""
    th2, two, rho2 = _consts(o)
    n = len(X); pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    i, j = pairs[:, 0], pairs[:, 1]
    ok0 = (i != j) & (i >= 0) & (j >= 0) & (i < n) & (j < n)
    ii, jj = np.where(ok0, i, 0), np.where(ok0, j, 0)
    Xk = _conv(X, kind); Yk = _conv(Y, kind)
    half = _conv(2.0, kind)
    with np.errstate(all="ignore"):
        Xi = [Xk[ii, k] for k in range(3)]; Xj = [Xk[jj, k] for k in range(3)]; Yi = [Yk[ii, k] for k in range(3)]; Yj = [Yk[jj, k] for k in range(3)]
        a = [Xi[k] - Xj[k] for k in range(3)]; b = [Yi[k] - Yj[k] for k in range(3)]
        ra2 = a[0] * a[0] + a[1] * a[1]; rb2 = b[0] * b[0] + b[1] * b[1]
        ok1 = ok0 & (_v(ra2) > rho2) & (_v(rb2) > rho2)
        dz = _abs(a[2] - b[2])
        ok2 = ok1 & ~(_v(dz) > two)
        safe = lambda x: x if kind != "v" else V(np.where(ok1, x.v, 1), np.where(ok1, x.e, 0))
        dl = _abs(_sqrt(safe(ra2)) - _sqrt(safe(rb2)))
        ok3 = ok2 & ~(_v(dl) > two)
        dot = a[0] * b[0] + a[1] * b[1]; crs = a[0] * b[1] - a[1] * b[0]
        nn = dot * dot + crs * crs
        nrm = _sqrt(nn if kind != "v" else V(np.where(ok3, nn.v, 1), np.where(ok3, nn.e, 0)))
        valid = ok3 & (_v(nrm) > 0)
        c = dot / nrm; s = crs / nrm
        qi0 = c * Xi[0] - s * Xi[1]; qi1 = s * Xi[0] + c * Xi[1]
        qj0 = c * Xj[0] - s * Xj[1]; qj1 = s * Xj[0] + c * Xj[1]
        t = [((Yi[0] - qi0) + (Yj[0] - qj0)) / half, ((Yi[1] - qi1) + (Yj[1] - qj1)) / half, ((Yi[2] - Xi[2]) + (Yj[2] - Xj[2])) / half]
    flagged = _near(ra2, rho2, ok0) + _near(rb2, rho2, ok0) + _near(dz, two, ok1) + _near(dl, two, ok2)
    reason = np.full(len(pairs), R_MODEL)
    for cond, code in ((ok2 & ~ok3, R_LENGTH), (ok1 & ~ok2, R_DZ), (ok0 & ~ok1, R_RHO), (~ok0, R_INDEX)):
        reason[cond] = code
    return dict(valid=valid, c=c, s=s, t=t, reason=reason, flagged=flagged)


def residual2(c, s, t, Xk, Yk):
    """d2 of the score for models (c, s (M, 1), t three (M, 1)) on matches (Xk, Yk: three (1, n) each)"""
    q0 = c * Xk[0] - s * Xk[1]; q1 = s * Xk[0] + c * Xk[1]
    dx = (q0 + t[0]) - Yk[0]; dy = (q1 + t[1]) - Yk[1]; dz = (Xk[2] + t[2]) - Yk[2]
    return (dx * dx + dy * dy) + dz * dz


def score(sv, X, Y, o, kind, only=None):
    """inlier flags (M, n) of the valid models (or of the hypotheses `only`), their hypothesis indices, and the flagged inlier tests"""
    th2, _, _ = _consts(o)
    hs = np.nonzero(sv["valid"])[0] if only is None else np.asarray(only, np.int64)
    Xk = [_conv(X[:, k], kind)[None, :] for k in range(3)]; Yk = [_conv(Y[:, k], kind)[None, :] for k in range(3)]
    inl = np.zeros((len(hs), len(X)), bool); flagged = 0
    for lo in range(0, len(hs), 128):
        sl = hs[lo:lo + 128]
        col = lambda x: x[sl][:, None] if not isinstance(x, V) else V(x.v[sl][:, None], x.e[sl][:, None])
        with np.errstate(all="ignore"):
            d2 = residual2(col(sv["c"]), col(sv["s"]), [col(x) for x in sv["t"]], Xk, Yk)
            inl[lo:lo + 128] = _v(d2) <= th2
        flagged += _near(d2, th2, np.ones(_v(d2).shape, bool))
    return inl, hs, flagged


def refine(cw, sw, tw, X, Y, kind):
    """the closed form over the matches given (the winner's inliers) -> dict(status, c, s, t, A, rms, sing: (nrm, its threshold))"""
    m = len(X)
    Xk = [_conv(X[:, k], kind) for k in range(3)]; Yk = [_conv(Y[:, k], kind) for k in range(3)]
    cnt = _conv(float(m), kind); two = _conv(2.0, kind)
    mX = [_sum(x) / cnt for x in Xk]; mY = [_sum(y) / cnt for y in Yk]
    x = [Xk[k] - mX[k] for k in range(2)]; y = [Yk[k] - mY[k] for k in range(2)]
    D = _sum(x[0] * y[0] + x[1] * y[1]); C = _sum(x[0] * y[1] - x[1] * y[0])
    W = _sum((x[0] * x[0] + x[1] * x[1]) + (y[0] * y[0] + y[1] * y[1]))
    nrm = _sqrt(D * D + C * C) if float(_v(D * D + C * C)) > 0 else (D * D + C * C)
    lim = (W / two) * _conv(SING_REL, kind)
    ok = bool(_v(nrm) > _v(lim))
    c, s, t, status = cw, sw, list(tw), SINGULAR
    if ok:
        status = OK
        c = D / nrm; s = C / nrm
        t = [mY[0] - (c * mX[0] - s * mX[1]), mY[1] - (s * mX[0] + c * mX[1]), mY[2] - mX[2]]
    q0 = c * Xk[0] - s * Xk[1]; q1 = s * Xk[0] + c * Xk[1]
    rx = (q0 + t[0]) - Yk[0]; ry = (q1 + t[1]) - Yk[1]; rz = (Xk[2] + t[2]) - Yk[2]
    zero = _conv(0.0, kind)
    A = [[zero] * 4 for _ in range(4)]
    A[0][0] = _sum(q1 * q1 + q0 * q0); A[0][1] = A[1][0] = _sum(-q1); A[0][2] = A[2][0] = _sum(q0); A[1][1] = A[2][2] = A[3][3] = cnt
    rms = _sqrt(_sum((rx * rx + ry * ry) + rz * rz) / cnt) if float(_v(_sum((rx * rx + ry * ry) + rz * rz))) > 0 else zero
    return dict(status=status, c=c, s=s, t=t, A=A, rms=rms, sing=(nrm, lim))


def run(X, Y, pairs, opt=None, kind="ld", mutate=None):
    """lvk_align_ransac_3d on n = len(X) matches and the pairs given.  -> dict: n_models, count (P,), c, s (P,), t (P, 3) (zero without a
    model), reason, status, hyp, n_inliers, mask, min_model and model (c, s, t), A (4, 4), rms.  mutate: None, "sign_s" (s negated),
    "tie_high" (ties to the highest index), "no_z" (the score leaves d_z out)"""
    assert kind in ("ld", "f64")
    o = options(**(opt or {}))
    X = np.asarray(X, np.float64).reshape(-1, 3); Y = np.asarray(Y, np.float64).reshape(-1, 3)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n, P = len(X), len(pairs)
    dt = np.float64 if kind == "f64" else LD
    out = dict(n_models=np.zeros(P, np.int32), count=np.zeros(P, np.int64), c=np.zeros(P, dt), s=np.zeros(P, dt), t=np.zeros((P, 3), dt), reason=np.full(P, R_INDEX),
               mask=np.zeros(n, np.uint8), status=NO_MODEL, hyp=-1, n_inliers=0, tie=False, min_model=(dt(1), dt(0), np.zeros(3, dt)), model=(dt(1), dt(0), np.zeros(3, dt)),
               A=np.zeros((4, 4), dt), rms=dt(0))
    if n < 2 or P == 0:
        return out
    sv = solve(X, Y, pairs, o, kind)
    if mutate == "sign_s":
        sv["s"] = -sv["s"]
    out["reason"] = sv["reason"]
    valid = sv["valid"]
    if not valid.any():
        return out
    if mutate == "no_z":                                 # d_z left out: every match's z "agrees"
        Xs = X.copy(); Xs[:, 2] = 0.0; Ys = Y.copy(); Ys[:, 2] = 0.0
        sv2 = dict(sv); sv2["t"] = [sv["t"][0], sv["t"][1], sv["t"][2] * 0]
        inl, hs, _ = score(sv2, Xs, Ys, o, kind)
    else:
        inl, hs, _ = score(sv, X, Y, o, kind)
    cnt = inl.sum(1)
    out["n_models"] = valid.astype(np.int32); out["count"][hs] = cnt
    out["c"][hs] = sv["c"][hs]; out["s"][hs] = sv["s"][hs]
    for k in range(3):
        out["t"][hs, k] = sv["t"][k][hs]
    best = int(cnt.max())
    w = int(np.argmax(cnt)) if mutate != "tie_high" else int(len(cnt) - 1 - np.argmax(cnt[::-1]))
    h = int(hs[w])
    cw, sw, tw = out["c"][h], out["s"][h], out["t"][h].copy()
    out.update(tie=bool((cnt == best).sum() > 1), hyp=h, n_inliers=best, mask=inl[w].astype(np.uint8), min_model=(cw, sw, tw), model=(cw, sw, tw.copy()))
    if best < o["min_inliers"]:
        out["status"] = FEW_INLIERS
        return out
    sel = inl[w]
    rf = refine(cw, sw, [tw[0], tw[1], tw[2]], X[sel], Y[sel], kind)
    out.update(status=rf["status"], model=(rf["c"], rf["s"], np.array(rf["t"], dt)), A=np.array(rf["A"], dt), rms=rf["rms"])
    return out


DISCRETE = ("n_models", "count", "reason", "mask", "status", "hyp", "n_inliers")


def same_discrete(a, b):
    """the names of the discrete results in which two runs differ"""
    return [k for k in DISCRETE if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def decisions(X, Y, pairs, ref, opt=None):
    """the number of deciding comparisons that lie inside their V bound (see the module's text); ref = run(.., kind="ld")"""
    o = options(**(opt or {}))
    X = np.asarray(X, np.float64).reshape(-1, 3); Y = np.asarray(Y, np.float64).reshape(-1, 3)
    if len(X) < 2 or len(np.asarray(pairs).reshape(-1, 2)) == 0:
        return 0
    sv = solve(X, Y, pairs, o, "v")
    flagged = sv["flagged"]
    assert np.array_equal(sv["valid"], ref["n_models"].astype(bool))
    if sv["valid"].any():
        _, _, f = score(sv, X, Y, o, "v")
        flagged += f
    if ref["status"] in (OK, SINGULAR):
        sel = ref["mask"].astype(bool); h = ref["hyp"]
        rf = refine(sv["c"][h], sv["s"][h], [x[h] for x in sv["t"]], X[sel], Y[sel], "v")
        nrm, lim = rf["sing"]
        e = LD(nrm.e) + LD(lim.e)
        flagged += int(e > 0 and abs(LD(nrm.v) - LD(lim.v)) <= 2 * e)
    return flagged


def bounds(X, Y, pairs, ref, opt=None):
    """The tolerances of the GPU comparison of the refined results against `ref` = run(.., kind="ld") -> dict(model (5,): c, s, t; A (4, 4); rms).
    The winner (c0, s0, t0) and every hypothesis are compared bit for bit with the float64 run and need none; where the winner is what
    A and rms are evaluated at (SINGULAR), it enters with the error its own solve carries."""
    out = dict(model=np.zeros(5, LD), A=np.zeros((4, 4), LD), rms=LD(0))
    if ref["status"] not in (OK, SINGULAR):
        return out
    X = np.asarray(X, np.float64).reshape(-1, 3); Y = np.asarray(Y, np.float64).reshape(-1, 3)
    extra = 2 * (1 + U_LD / U)                           # doubled, and this file's own rounding of the same expressions
    sel = ref["mask"].astype(bool)
    sv = solve(X, Y, np.asarray(pairs, np.int64).reshape(-1, 2)[[ref["hyp"]]], options(**(opt or {})), "v")
    rf = refine(sv["c"][0], sv["s"][0], [x[0] for x in sv["t"]], X[sel], Y[sel], "v")
    if ref["status"] == OK:
        out["model"] = extra * np.array([rf["c"].e, rf["s"].e, *[x.e for x in rf["t"]]], LD)
    out["A"] = extra * np.array([[LD(a.e) if isinstance(a, V) else LD(0) for a in row] for row in rf["A"]], LD)
    out["rms"] = extra * LD(rf["rms"].e) if isinstance(rf["rms"], V) else LD(0)
    return out


def gauss_newton(c, s, t, X, Y, iters=20):
    """plain Gauss-Newton on (psi, t) from (c, s, t), minimising sum |Rz X + t - Y|^2, long double - what the closed form is held to"""
    psi = np.arctan2(LD(s), LD(c)); t = np.asarray(t, LD).copy()
    X = np.asarray(X, LD); Y = np.asarray(Y, LD)
    for _ in range(iters):
        cc, ss = np.cos(psi), np.sin(psi)
        q = np.stack([cc * X[:, 0] - ss * X[:, 1], ss * X[:, 0] + cc * X[:, 1], X[:, 2]], -1)
        r = q + t - Y
        J = np.zeros((len(X), 3, 4), LD)
        J[:, 0, 0] = -q[:, 1]; J[:, 1, 0] = q[:, 0]; J[:, 0, 1] = J[:, 1, 2] = J[:, 2, 3] = 1
        A = np.einsum("nki,nkj->ij", J, J); g = np.einsum("nki,nk->i", J, r)
        d = np.linalg.solve(A.astype(np.float64), -g.astype(np.float64)).astype(LD)
        psi = psi + d[0]; t = t + d[1:]
    return np.cos(psi), np.sin(psi), t
