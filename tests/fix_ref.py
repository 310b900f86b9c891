"""Long-double restatement of what lvk_ekf_update_sparse and lvk_ekf_add_fix (include/lvk_c.h) define.

The update, for a measurement of m rows on the columns `cols` of an n x n covariance P, with noise covariance R:
    S = H P[cols, cols] H^T + R = L L^T,   gamma = r^T S^-1 r,   W = L^-1 H P[cols, :],   dx = W^T L^-1 r,   P <- P - W^T W,
status 0 applied, 1 gated out (gate > 0 and not gamma <= gate), 2 S not positive definite; with status 1 or 2 dx = 0 and P stays.

The measurement models, under the filter's state injection (attitude q <- small_angle_quat(d_theta) * q, i.e. R <- (I + [d_theta]x) R,
position p <- p + d_p; a clone's six columns are [d_theta d_p]):
    position fix on clone i, lever arm l in the body frame:   prediction p_i + R_i l,   H_theta = -[R_i l]x,   H_p = I
    ... between adjacent clones i, j with weight a:           (1 - a)(p_i + R_i l) + a (p_j + R_j l),   blocks scaled by 1 - a and a
    pose fix: three rows in front,   r_theta = 2 vec(q_z * q_i^-1) with w >= 0,   H_theta = I on clone i.

Two routes to H: jacobian_nd(), central differences of the prediction under the injection, written from the geometry (no derivative
is written down on that route), and the closed form (fix_rows()), carried - like the update (update_tracked()) - through a first-order
running error analysis of the float64 operations the library performs (class V of tests/msckf_point_ref.py).
tests/test_fix_ref.py holds the routes to each other; the GPU tests compare the kernels with the long-double value inside the bound.

A pose is (col, q, p): the first of the clone's six columns, its attitude [x y z w] (body to world) and position."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, quat_mul, small_angle_quat, skew
from tests.msckf_point_ref import V, _V, mm, stack, skew_v, quat_to_rot_v, LD, U, U_LD
from tests.pose_rel_ref import inject, filter_like_cov, with_gauge, random_slot, buffer      # noqa: F401  (buffer: used by the GPU tests)

H_STEP = LD(2.0) ** -21           # central-difference step, as pose_rel_ref.H_STEP
# The closed-form H against the central-difference H, entrywise, relative to (1 + |l|) (the size of the functions differentiated: a
# position offset by a rotated lever arm, and a rotation vector).  Truncation: h^2 f''' / 6 = 3.8e-14 f''', f''' <= a few (1 + |l|) (every
# derivative of a rotation keeps its norm).  Rounding: ~50 long-double operations, 50 * 2^-64 (1 + |l| + |p|), divided by 2 h = 9.5e-7:
# 3e-12 (1 + |l| + |p|), |p| <= 5 here.  1e-10 leaves a factor 5 and more, as in the siblings.
TOL_ND = 1e-10
CHI2_005 = {3: 0.35184631774927144, 6: 1.6353828943279067}      # the filter's own table (chi2_table.inc): the 5 % quantiles
POSITION, POSE = 0, 1


def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ the geometry
def predict_position(poses, a, lever, deltas=None):
    """(1 - a)(p_i + R_i l) + a (p_j + R_j l) (one pose: p_i + R_i l) after the injection of deltas[k] = [d_theta d_p] into pose k"""
    out = np.zeros(3, LD)
    w = [LD(1)] if len(poses) == 1 else [1 - LD(a), LD(a)]
    for k, (_, q, p) in enumerate(poses):
        qk, pk = inject(q, p, np.zeros(6, LD) if deltas is None else deltas[k])
        out = out + w[k] * (pk + quat_to_rot(qk) @ _ld(lever))
    return out


def attitude_error(q_z, q):
    """2 vec(q_z * q^-1), the sign taken so that w >= 0"""
    q = np.asarray(q, LD)
    dq = quat_mul(np.asarray(q_z, LD), np.array([-q[0], -q[1], -q[2], q[3]], LD))
    return (-2 if dq[3] < 0 else 2) * dq[0:3]


def jacobian_nd(kind, poses, a, lever, h=H_STEP):
    """m x 6 len(poses): central differences, under the injection, of the position prediction and - POSE - of minus the attitude
    error of the clone against its own unperturbed attitude (the residual's derivative with the sign of a prediction's)"""
    k6 = 6 * len(poses)
    rows = []
    for k in range(k6):
        col = []
        for sgn in (1, -1):
            d = np.zeros(k6, LD); d[k] = sgn * h
            deltas = [d[6 * s:6 * s + 6] for s in range(len(poses))]
            f = predict_position(poses, a, lever, deltas)
            if kind == POSE:
                qi, _ = inject(poses[0][1], poses[0][2], deltas[0])
                f = np.concatenate([-attitude_error(poses[0][1], qi), f])
            col.append(f)
        rows.append((col[0] - col[1]) / (2 * h))
    return np.array(rows, LD).T


def fix_rows(kind, poses, a, lever, z_p, z_q=None, mutate=None):
    """-> (cols, H, r): the columns and, as V (value in long double, bound on the error of the library's float64 host code, which this
    follows operation by operation), H (m x 6 len(poses)) and r of a fix.  mutate: None, "sign" (the sign of [R l]x) or "swap_a" (a and
    1 - a swapped)"""
    pose = kind == POSE
    m, nc, row0 = (6 if pose else 3), 6 * len(poses), (3 if pose else 0)
    Hv = np.zeros((m, nc), LD); He = np.zeros((m, nc), LD)
    lev = V(_ld(lever))
    pred = None
    cols = []
    w_i, w_j = V(LD(1)) - V(LD(a)), V(LD(a))
    if mutate == "swap_a":
        w_i, w_j = w_j, w_i
    for s, (col, q, p) in enumerate(poses):
        wgt = V(LD(1)) if len(poses) == 1 else (w_j if s else w_i)
        Rl = mm(quat_to_rot_v(q), lev)
        Sk = skew_v(Rl)
        if mutate == "sign":
            Sk = -Sk
        term = wgt * (V(_ld(p)) + Rl)
        pred = term if pred is None else pred + term
        blk = wgt * (-Sk)
        Hv[row0:row0 + 3, 6 * s:6 * s + 3] = blk.v; He[row0:row0 + 3, 6 * s:6 * s + 3] = blk.e
        for x in range(3):
            Hv[row0 + x, 6 * s + 3 + x] = wgt.v; He[row0 + x, 6 * s + 3 + x] = wgt.e
        cols += list(range(col, col + 6))
    rp = V(_ld(z_p)) - pred
    rv = np.zeros(m, LD); re = np.zeros(m, LD)
    rv[row0:] = rp.v; re[row0:] = rp.e
    if pose:
        qi = _ld(poses[0][1])
        ax, ay, az, aw = (V(c) for c in _ld(z_q)); bx, by, bz, bw = V(-qi[0]), V(-qi[1]), V(-qi[2]), V(qi[3])
        dw = aw * bw - ax * bx - ay * by - az * bz
        dq = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx]
        sg = LD(-2) if dw.v < 0 else LD(2)
        for x in range(3):
            rv[x] = sg * dq[x].v; re[x] = 2 * dq[x].e
            Hv[x, x] = 1
    return np.array(cols), V(Hv, He), V(rv, re)


# ------------------------------------------------------------------------------------------------ the update, plainly
def chol(S):
    """lower Cholesky factor in the arithmetic of S; None when a pivot is not > 0"""
    m = S.shape[0]; L = np.zeros_like(S)
    for j in range(m):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            L[i, j] = (S[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def fsub(L, B):
    """L^-1 B by forward substitution"""
    X = np.zeros_like(B)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def update(P, cols, H, r, R, gate=0.0, mutate=None):
    """the definition in long double -> dict(status, gamma, dx, P, S).  mutate: None, "no_R" (R left out of S) or "swap_cols" (within every
    block of six columns the d_theta and d_p columns swapped)"""
    P = _ld(P); H = np.asarray(_V(H).v, LD); r = np.asarray(_V(r).v, LD); R = _ld(R)
    cols = np.asarray(cols)
    if mutate == "swap_cols":
        cols = cols.reshape(-1, 6)[:, [3, 4, 5, 0, 1, 2]].ravel()
    S = H @ P[np.ix_(cols, cols)] @ H.T + (0 if mutate == "no_R" else R)
    L = chol(S)
    out = dict(status=0, gamma=LD(0), dx=np.zeros(P.shape[0], LD), P=P, S=S)
    if L is None:
        out["status"] = 2
        return out
    y = fsub(L, r)
    out["gamma"] = y @ y
    if gate > 0 and not out["gamma"] <= gate:
        out["status"] = 1
        return out
    W = fsub(L, H @ P[cols, :])
    out["dx"] = W.T @ y; out["P"] = P - W.T @ W
    return out


# ------------------------------------------------------------------------------------------------ running error analysis
def vsqrt(x):
    s = np.sqrt(x.v)
    return V(s, x.e / (2 * s) + U * s)


def update_tracked(P, cols, H, r, R, gate=0.0):
    """-> dict(status, gamma, dx, P, e_gamma, e_dx, e_P, pmin): the long-double update with the derived componentwise bounds on the
    error of the two kernels (be_fix.hip) against it.  H and r may be V: what they carry is propagated.

    The bounds are first order in u = 2^-53 and follow the kernels operation by operation (class V: every operation adds the rounding of
    its own result - u |result|, gamma_k |a| |b| for an inner product of length k - to what its operands carry): T_s = H P_s and
    S = T_s H^T, inner products of length ncols, and one addition of R; the Cholesky factorisation entry by entry - a running difference
    of products, a square root (u on top of half the relative error of its argument), a division - so that the conditioning of S enters
    through the divisions by L_ii exactly where the kernel meets it; y = L^-1 r and gamma = y^T y as running sums; for every column
    t = H P[cols, j] (length ncols), w by forward substitution, dx_j = sum_i w_i y_i; then s = sum_i W[i][a] W[i][b] and P - s.  The whole
    is doubled for the terms of higher order, and this file's own rounding (u_ld / u of the same expression, and u_ld per term of the
    entrywise scale) is added.  Nothing in it is fitted to a result."""
    P = _ld(P); H = _V(H); r = _V(r); R = _ld(R); cols = np.asarray(cols)
    n = P.shape[0]; m = H.v.shape[0]
    S = mm(mm(H, V(P[np.ix_(cols, cols)])), H.T) + V(R)
    Sv = np.triu(S.v) + np.triu(S.v, 1).T; Se = np.triu(S.e) + np.triu(S.e, 1).T      # the kernel forms the upper triangle and mirrors it
    Sm = [[V(Sv[i, j], Se[i, j]) for j in range(m)] for i in range(m)]
    out = dict(status=0, gamma=LD(0), e_gamma=LD(0), dx=np.zeros(n, LD), e_dx=np.zeros(n, LD), P=P, e_P=np.zeros((n, n), LD), pmin=None)
    L = [[None] * m for _ in range(m)]
    for j in range(m):
        d = Sm[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d.v > 0:
            out["status"] = 2; out["pmin"] = d.v
            return out
        out["pmin"] = d.v if out["pmin"] is None else min(out["pmin"], d.v)
        L[j][j] = vsqrt(d)
        for i in range(j + 1, m):
            s = Sm[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    y = []
    for i in range(m):
        s = r[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y.append(s / L[i][i])
    g = V(LD(0))
    for i in range(m):
        g = g + y[i] * y[i]
    fin = lambda e, scale: 2 * e * (1 + U_LD / U) + 24 * U_LD * scale
    out["gamma"] = g.v; out["e_gamma"] = fin(g.e, g.v)
    if gate > 0 and not g.v <= gate:
        out["status"] = 1
        return out
    T = mm(H, V(P[cols, :]))
    w = []
    for i in range(m):
        s = T[i]
        for k in range(i):
            s = s - L[i][k] * w[k]
        w.append(s / L[i][i])
    dx = V(np.zeros(n, LD)); s_dx = np.zeros(n, LD)
    G = V(np.zeros((n, n), LD)); s_P = np.abs(P)
    for i in range(m):
        dx = dx + w[i] * y[i]; s_dx = s_dx + np.abs(w[i].v * y[i].v)
        G = G + V(w[i].v[:, None], w[i].e[:, None]) * V(w[i].v[None, :], w[i].e[None, :]); s_P = s_P + np.abs(np.outer(w[i].v, w[i].v))
    Pn = V(P) - G
    out["dx"] = dx.v; out["e_dx"] = fin(dx.e, s_dx); out["P"] = Pn.v; out["e_P"] = fin(Pn.e, s_P)
    return out


def whitened_update(P, cols, H, r, R, sigma2=LD(6.4e-5)):
    """the route update_zupt takes (be_prune.hip): the rows whitened to the isotropic sigma2 - here with the Cholesky factor of a full R,
    which for a diagonal R is update_zupt's scaling by sqrt(sigma2 / R_ii) - then the dense isotropic update -> (dx, P)"""
    P = _ld(P); n = P.shape[0]
    Hd = np.zeros((H.shape[0], n), LD); Hd[:, np.asarray(cols)] = np.asarray(H, LD)
    LR = chol(_ld(R)); sg = np.sqrt(LD(sigma2))
    Hw = sg * fsub(LR, Hd); rw = sg * fsub(LR, np.asarray(r, LD))
    L = chol(Hw @ P @ Hw.T + LD(sigma2) * np.eye(H.shape[0], dtype=LD))
    W = fsub(L, Hw @ P)
    return W.T @ fsub(L, rw), P - W.T @ W


# ------------------------------------------------------------------------------------------------ test problems
PAD = 5
_PROBLEMS = None


def _spd(rng, m, lo, hi):
    """a full m x m covariance with standard deviations in [lo, hi]"""
    A = rng.normal(0, 1, (m, m + 2)); C = A @ A.T
    s = 1 / np.sqrt(np.diag(C)); C = C * s[:, None] * s[None, :]
    D = rng.uniform(lo, hi, m)
    R = C * D[:, None] * D[None, :]
    return (R + R.T) / 2


def make_problem(name, seed, n_clones, n, ldp, kind, ranks=(), a=0.0, lever=False, gate=0.0, off=0.0, generic=None, leg=22):
    """P = D C D with variances log-uniform over 1e-8 .. 1 plus a gauge component of variance 1e2 over the IMU pose and every clone
    (pose_rel_ref's recipe).  kind POSITION / POSE: a fix on the clones `ranks` (two: interpolated with weight a), lever arm zero or of
    0.3 m, z = the prediction + N(0, R) + off along x, R full with sigmas 0.05 .. 0.5 (m, rad).  generic = (m, cols): a random H on
    those columns instead.  The library gets H and r rounded to float64: they are the problem's inputs."""
    rng = np.random.default_rng([20261020, seed])
    imu = random_slot(rng, 0, 6)
    clones = [random_slot(rng, leg + 6 * c, leg + 6 * c + 3) for c in range(n_clones)]
    P = with_gauge(filter_like_cov(rng, n), [imu] + clones)
    pr = dict(name=name, n=n, ldp=ldp, P=P, kind=kind, a=a, gate=gate, generic=generic is not None)
    if generic is not None:
        m, cols = generic
        pr.update(cols=np.array(cols), H=rng.normal(0, 1, (m, len(cols))), r=rng.normal(0, 0.1, m) + off, R=_spd(rng, m, 0.05, 0.5), lever=np.zeros(3), poses=None)
        return pr
    m = 6 if kind == POSE else 3
    poses = [(clones[k][0], clones[k][2], clones[k][3]) for k in ranks]
    lv = rng.normal(0, 1, 3) if lever else np.zeros(3)
    if lever:
        lv *= 0.3 / np.linalg.norm(lv)
    R = _spd(rng, m, 0.05, 0.5)
    noise = np.linalg.cholesky(R) @ rng.normal(0, 1, m)
    z_p = (predict_position(poses, a, lv).astype(np.float64) + noise[m - 3:] + np.array([off, 0, 0]))
    z_q = None
    if kind == POSE:
        z_q = quat_mul(small_angle_quat(_ld(noise[:3])), _ld(poses[0][1])).astype(np.float64)
    cols, H, r = fix_rows(kind, poses, a, lv, z_p, z_q)
    pr.update(cols=cols, H=H.v.astype(np.float64), r=r.v.astype(np.float64), R=R, lever=lv, poses=poses, z_p=z_p, z_q=z_q)
    return pr


def stage_problems():
    """Every problem the GPU stage tests run, built once: n = 28, 34, 63, 64, 65 and 433, ldp = n and n + PAD, m = 3 and 6, ncols 3, 6
    and 12, the first three and the last six columns of P, a in {0, 0.5, 1} (and 0.25), zero and non-zero lever arm, two gated problems."""
    global _PROBLEMS
    if _PROBLEMS is not None:
        return _PROBLEMS
    g3, g6 = CHI2_005[3], CHI2_005[6]
    _PROBLEMS = [
        make_problem("n28 position", 1, 1, 28, 28, POSITION, (0,)),                                  # the last six columns of P
        make_problem("n28 pose lever", 2, 1, 28, 28 + PAD, POSE, (0,), lever=True, gate=100 * g6),
        make_problem("n28 first three", 3, 1, 28, 28, POSITION, generic=(3, (0, 1, 2))),
        make_problem("n34 a=.5 lever", 4, 2, 34, 34 + PAD, POSITION, (0, 1), a=0.5, lever=True),
        make_problem("n34 a=0", 5, 2, 34, 34, POSITION, (0, 1), a=0.0, gate=100 * g3),
        make_problem("n34 a=1 lever", 6, 2, 34, 34 + PAD, POSITION, (0, 1), a=1.0, lever=True),
        make_problem("n63 position lever", 7, 6, 63, 63, POSITION, (3,), lever=True),
        make_problem("n64 pose", 8, 6, 64, 64 + PAD, POSE, (5,)),
        make_problem("n65 m6 first three", 9, 6, 65, 65, POSE, generic=(6, (0, 1, 2))),
        make_problem("n65 a=.25 lever", 10, 6, 65, 65 + PAD, POSITION, (2, 3), a=0.25, lever=True),
        make_problem("n433 a=.5 lever", 11, 62, 433, 433, POSITION, (30, 31), a=0.5, lever=True),
        make_problem("n433 pose lever", 12, 62, 433, 433 + PAD, POSE, (61,), lever=True),
        make_problem("n433 gated", 13, 62, 433, 433 + PAD, POSITION, (0,), gate=g3, off=100.0),
        make_problem("n65 gated m6", 14, 6, 65, 65, POSE, (1,), lever=True, gate=g6, off=100.0),
        make_problem("n433 m6 twelve", 15, 62, 433, 433, POSE, generic=(6, (3, 4, 5, 100, 101, 250, 427, 428, 429, 430, 431, 432))),
    ]
    return _PROBLEMS


def record(pr, fill=0.0, R=None, gate=None):
    """the stage entry's record of a problem"""
    from larvio_amd.ops import sparse_update_record
    return sparse_update_record(pr["cols"], pr["H"], pr["r"], pr["R"] if R is None else R, pr["gate"] if gate is None else gate, fill=fill)


# ------------------------------------------------------------------------------------------------ the filter's window
def clone_pose(clone, rank, leg=22):
    return (leg + 6 * rank, np.array(clone["q"], np.float64), np.array(clone["p"], np.float64))


def worst_ratio(diff, bound):
    """max |diff| / bound over the entries; an entry whose bound is 0 (an exact zero of the restatement: nothing was added up) must be 0 too"""
    diff = np.abs(np.asarray(diff, LD)); bound = np.asarray(bound, LD) + np.zeros(diff.shape, LD)
    zero = bound == 0
    if np.any(diff[zero] != 0):
        return np.inf
    return float(np.max(diff[~zero] / bound[~zero])) if np.any(~zero) else 0.0
