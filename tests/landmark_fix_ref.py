"""Long-double restatement of what lvk_ekf_update_landmarks and lvk_ekf_add_landmark_obs (include/lvk_c.h) define.

A batch is the set of observations made in one image, i.e. of one clone b (attitude q_b body to world, position p_b, columns c..c+5
= [d_theta_b d_p_b]); the extrinsics (R_b2c, t_c_b) have columns 15..20 = [d_theta_e d_t].  For a world point p_w with covariance
Sigma_w, a normalised observation z = (u, v) and noise sigma:
    g = p_w - p_b,   y = R_b^T g - t_c_b,   p_c = R_b2c y,   h = (p_c.x / p_c.z, p_c.y / p_c.z),   r = z - h,
    M = R_b2c R_b^T,   d p_c = [R_b2c [y]x | -R_b2c | M [g]x | -M],   H = J_pi d p_c (2 x 12),   R_k = sigma^2 I + J_pi M Sigma_w M^T J_pi^T,
under the filter's injection (R_b <- (I + [d_theta_b]x) R_b, p_b <- p_b + d_p_b, R_b2c <- R_b2c R(d_theta_e)^T, t_c_b <- t_c_b + d_t).
On the covariance as it is before the batch: p_c.z <= min_depth is BEHIND; gamma_k = r^T (H P_s H^T + R_k)^-1 r, USED iff gate <= 0 or
gamma_k <= gate, else GATED; used rows are whitened by the Cholesky factor of R_k, stacked, compressed when there are more than 12 rows
- to as many rows as they have rank, 6 for points in general position: all twelve columns act through the camera's pose - and applied:  S = H P_s H^T + I = L L^T,  W = L^-1 H P[cols, :],  dx = W^T L^-1 r,  P <- P - W^T W.

Two routes to H: jacobian_nd(), central differences of h under the injection, written from the geometry (no derivative is written down
on that route), and the closed form (obs_rows()), carried - like everything behind it (batch_tracked()) - through a first-order running
error analysis of the float64 operations the kernels perform (class V of tests/msckf_point_ref.py; the last two launches are the
update of tests/fix_ref.py with unit noise and up to twelve rows).  batch_plain() is the definition written down literally, without
whitening or compression.  tests/test_landmark_fix_ref.py holds the routes to each other; the GPU tests compare the kernels with the
long-double value inside the bound."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, quat_mul, small_angle_quat, skew
from tests.msckf_point_ref import V, _V, mm, stack, hcat, skew_v, quat_to_rot_v, LD, U, U_LD
from tests.pose_rel_ref import filter_like_cov, with_gauge, random_slot, buffer      # noqa: F401  (buffer: used by the GPU tests)
from tests import fix_ref as F

H_STEP = LD(2.0) ** -21           # central-difference step, as pose_rel_ref.H_STEP
# The closed-form H against the central-difference H, entrywise, relative to (1 + |g|) / z (the size of the function differentiated: a
# projection of a point |g| away at depth z).  Truncation: h^2 f''' / 6 = 3.8e-14 f''', f''' <= a few dozen times that size at the
# depths used (z >= 1.5: every derivative of 1/z costs at most 1/1.5).  Rounding: ~60 long-double operations, 60 * 2^-64 (1 + |g| + |p|),
# divided by 2 h = 9.5e-7: 4e-12 (1 + |g| + |p|), |p| <= 5 here.  1e-10 leaves a factor 5 and more, as in the siblings.
TOL_ND = 1e-10
CHI2_005_2 = 0.10258658877510106           # the filter's own table entry for 2 degrees of freedom (chi2_table.inc): the 5 % quantile
GATE_999 = 13.815510557964274 / CHI2_005_2   # gate_scale that makes the gate the 99.9 % quantile
USED, GATED, BEHIND = 0, 1, 2
MAX_OBS = 1024
# roundings on the path of one term of an inner product of the compression: the product, the lane's own addition, the wavefront's
# fixed tree (four row rotations, four row sums) and the sum over at most sixteen wavefronts
K_RED = 2 + 8 + 16
RANK_TOL2 = LD(2.0) ** -60        # be_landmark_fix.hip, LM_RANK_TOL2


def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


def make_job(clone_col, q_b, p_b, R_b2c, t_c_b, gate=0.0, min_depth=0.1):
    return dict(clone_col=int(clone_col), q_b=np.asarray(q_b, np.float64), p_b=np.asarray(p_b, np.float64), R_b2c=np.asarray(R_b2c, np.float64).reshape(3, 3),
                t_c_b=np.asarray(t_c_b, np.float64), gate=float(gate), min_depth=float(min_depth))


def columns(job, swap=False):
    """the twelve columns of P, ascending; swap: the mutation that takes the clone's d_p columns for d_theta and the other way round"""
    c = job["clone_col"]
    cl = [c + 3, c + 4, c + 5, c, c + 1, c + 2] if swap else list(range(c, c + 6))
    return np.array(list(range(15, 21)) + cl)


def sym_upper(c):
    c = _ld(c).reshape(3, 3)
    return np.triu(c) + np.triu(c, 1).T


# ------------------------------------------------------------------------------------------------ the geometry
def cam_point(job, p_w, d12=None):
    """p_c after the injection of d12 = [d_theta_e d_t d_theta_b d_p_b]"""
    d = np.zeros(12, LD) if d12 is None else np.asarray(d12, LD)
    q = quat_mul(small_angle_quat(d[6:9]), _ld(job["q_b"])); p = _ld(job["p_b"]) + d[9:12]
    Re = _ld(job["R_b2c"]) @ quat_to_rot(small_angle_quat(d[0:3])).T; t = _ld(job["t_c_b"]) + d[3:6]
    g = _ld(p_w) - p
    return Re @ (quat_to_rot(q).T @ g - t)


def project(pc):
    return np.array([pc[0] / pc[2], pc[1] / pc[2]], LD)


def jacobian_nd(job, p_w, h=H_STEP):
    """2 x 12: central differences of h under the injection"""
    J = np.zeros((2, 12), LD)
    for k in range(12):
        d = np.zeros(12, LD); d[k] = h
        J[:, k] = (project(cam_point(job, p_w, d)) - project(cam_point(job, p_w, -d))) / (2 * h)
    return J


def point_jacobian_nd(job, p_w, h=H_STEP):
    """2 x 3: central differences of h in p_w"""
    J = np.zeros((2, 3), LD)
    for k in range(3):
        d = np.zeros(3, LD); d[k] = h
        J[:, k] = (project(cam_point(job, _ld(p_w) + d)) - project(cam_point(job, _ld(p_w) - d))) / (2 * h)
    return J


# ------------------------------------------------------------------------------------------------ rows of one observation
def obs_rows(job, ob, mutate=None):
    """-> dict(status, pc, H (V 2 x 12), r (V 2), Rk (V 2 x 2), JM (V 2 x 3)) following the first kernel operation by operation; BEHIND
    carries nothing but status and pc.  mutate: None, "sign_g" (the sign of [g]x) or "no_cov" (Sigma_w left out of R_k)"""
    Rb = quat_to_rot_v(job["q_b"]); Re = V(_ld(job["R_b2c"]))
    M = mm(Re, Rb.T)
    g = V(_ld(ob["p_w"])) - V(_ld(job["p_b"]))
    y = mm(Rb.T, g) - V(_ld(job["t_c_b"]))
    pc = mm(Re, y)
    if not pc.v[2] > job["min_depth"]:
        return dict(status=BEHIND, pc=pc)
    Sg = skew_v(g)
    if mutate == "sign_g":
        Sg = -Sg
    D = hcat(hcat(mm(Re, skew_v(y)), -Re), hcat(mm(M, Sg), -M))
    x_, y_, z_ = pc[0], pc[1], pc[2]
    one = V(LD(1)); zero = V(LD(0))
    zz = z_ * z_
    dz = stack([[one / z_, zero, -(x_ / zz)], [zero, one / z_, -(y_ / zz)]])
    H = mm(dz, D); JM = mm(dz, M)
    r = V(_ld(ob["uv"])) - stack([x_ / z_, y_ / z_])
    sg = V(LD(ob["sigma"])); s2 = sg * sg
    Rk = mm(mm(JM, V(np.zeros((3, 3), LD) if mutate == "no_cov" else sym_upper(ob["cov_w"]))), JM.T) + V(np.eye(2, dtype=LD) * s2.v, np.eye(2, dtype=LD) * s2.e)
    return dict(status=USED, pc=pc, H=H, r=r, Rk=Rk, JM=JM)


def obs_gate_whiten(row, Ps, gate):
    """gamma_k (V), the status and the whitened 2 x 13 block (V) of one observation that is not behind"""
    H, r, Rk = row["H"], row["r"], row["Rk"]
    S = mm(mm(H, V(Ps)), H.T) + Rk
    S00, S01, S11 = S[0][0], S[0][1], S[1][1]
    gamma = V(LD(0)); st = GATED
    wa = F.vsqrt(Rk[0][0]) if Rk[0][0].v > 0 else None
    wb = Rk[0][1] / wa if wa is not None else None
    wc2 = Rk[1][1] - wb * wb if wa is not None else None
    if S00.v > 0 and wc2 is not None and wc2.v > 0:
        l00 = F.vsqrt(S00); l10 = S01 / l00; d = S11 - l10 * l10
        if d.v > 0:
            l11 = F.vsqrt(d); y0 = r[0] / l00; y1 = (r[1] - l10 * y0) / l11
            gamma = y0 * y0 + y1 * y1
            if not gate > 0 or gamma.v <= gate:
                st = USED
    if st != USED:
        return gamma, st, None
    wc = F.vsqrt(wc2)
    full = V(np.concatenate([H.v, r.v[:, None]], axis=1), np.concatenate([H.e, r.e[:, None]], axis=1))
    a0 = full[0] / wa
    a1 = (full[1] - wb * a0) / wc
    return gamma, st, V(np.stack([a0.v, a1.v]), np.stack([a0.e, a1.e]))


def compress_tracked(A):
    """the Householder reflections on [0; A], A a V of 2 n_used x 13: reflection j leaves the row R[j][j] = |a_j|, R[j][k] =
    a_j.a_k / |a_j| and a_k - (a_j.a_k / a_j.a_j) a_j.  The rank is decided as the kernel decides it: a column of which the reflections
    before it have left at most RANK_TOL2 of the squared norm it started with depends on them (the twelve columns act through the
    camera's pose: rank <= 6), and gives no reflection and no row -> (V m x 13, margin): m = rank rows, and the least factor by which a
    decision stood off RANK_TOL2 (tests/test_landmark_fix_ref.py asserts it large, so that float64 and long double decide alike).
    What is left of a dropped column is zero in exact arithmetic; it enters no later operation, so its rounding is carried nowhere.
    An inner product over the rows carries K_RED roundings per term whatever the order (the kernel's: lane, wavefront tree,
    wavefronts)."""
    Av = A.v.copy(); Ae = A.e.copy()
    c0 = np.sum(Av[:, :12] * Av[:, :12], axis=0)
    rows_v, rows_e = [], []; margin = np.inf
    for j in range(12):
        aj, ej = Av[:, j:j + 1], Ae[:, j:j + 1]
        tv = np.sum(aj * Av[:, j:], axis=0)
        te = np.sum(np.abs(aj) * Ae[:, j:] + ej * np.abs(Av[:, j:]), axis=0) + K_RED * U * np.sum(np.abs(aj * Av[:, j:]), axis=0)
        tot = V(tv, te)
        live = bool(tv[0] > RANK_TOL2 * c0[j])
        if c0[j] > 0:
            ratio = float(tv[0] / (RANK_TOL2 * c0[j]))
            margin = min(margin, ratio if live else (1 / ratio if ratio > 0 else np.inf))
        if not live:
            continue
        sig = tot[0]; nrm = F.vsqrt(sig)
        rv = np.zeros(13, LD); re = np.zeros(13, LD)
        rv[j] = nrm.v; re[j] = nrm.e
        rest = tot[1:]
        rj = rest / nrm; f = rest / sig
        rv[j + 1:] = rj.v; re[j + 1:] = rj.e
        upd = V(Av[:, j + 1:], Ae[:, j + 1:]) - V(f.v[None, :], f.e[None, :]) * V(aj, ej)
        Av[:, j + 1:] = upd.v; Ae[:, j + 1:] = upd.e
        rows_v.append(rv); rows_e.append(re)
    return V(np.array(rows_v, LD).reshape(-1, 13), np.array(rows_e, LD).reshape(-1, 13)), margin


# ------------------------------------------------------------------------------------------------ the batch
def batch_tracked(P, job, obs, mutate=None):
    """-> dict(status (n_obs,), gamma, e_gamma (n_obs,), info: batch status / n_used / n_gated / n_behind / m, gamma_b, e_gamma_b, pmin,
    dx, e_dx, P, e_P, depth_margin, H (the system's rows, V), r): the long-double batch with the derived componentwise bounds on the
    error of the three kernels (be_landmark_fix.hip) against it.

    The bounds are first order in u = 2^-53 and follow the kernels operation by operation (class V: every operation adds the rounding
    of its own result to what its operands carry): the rotation from the quaternion, M, g, y, p_c, the blocks of d p_c as inner
    products of length 3, J_pi, H and J_pi M, r, R_k; T = H P_s and S as inner products of length 12; the 2 x 2 Cholesky factor, gamma_k;
    the whitening (two square roots, a division per entry, one product and difference in the second row); the compression
    (compress_tracked); then the update of tests/fix_ref.py (update_tracked: S, its Cholesky factorisation entry by entry, y, W column
    by column, dx, the downdate) with R = I, which doubles the whole for the terms of higher order and adds this file's own rounding.
    Nothing in it is fitted to a result."""
    P = np.asarray(P, np.float64)
    n = P.shape[0]; cols = columns(job, swap=mutate == "swap_clone")
    Ps = P[np.ix_(cols, cols)].astype(LD)
    no = len(obs)
    status = np.zeros(no, int); gam = np.zeros(no, LD); e_gam = np.zeros(no, LD)
    blocks = []; margin = np.inf
    for k in range(no):
        row = obs_rows(job, obs[k], mutate if mutate in ("sign_g", "no_cov") else None)
        margin = min(margin, abs(float(row["pc"].v[2]) - job["min_depth"]) / max(job["min_depth"], 1e-300))
        if row["status"] == BEHIND:
            status[k] = BEHIND
            continue
        g, st, blk = obs_gate_whiten(row, Ps, job["gate"])
        status[k] = st; gam[k] = g.v; e_gam[k] = 2 * g.e * (1 + U_LD / U) + 24 * U_LD * g.v
        if st == USED:
            blocks.append(blk)
    n_used = len(blocks)
    out = dict(status=status, gamma=gam, e_gamma=e_gam, depth_margin=margin, n_used=n_used, n_gated=int(np.sum(status == GATED)), n_behind=int(np.sum(status == BEHIND)),
               m=min(2 * n_used, 12), batch_status=1, gamma_b=LD(0), e_gamma_b=LD(0), pmin=LD(0), dx=np.zeros(n, LD), e_dx=np.zeros(n, LD), P=P.astype(LD),
               e_P=np.zeros((n, n), LD), H=None, r=None, rank_margin=np.inf)
    if n_used == 0:
        return out
    A = V(np.concatenate([b.v for b in blocks]), np.concatenate([b.e for b in blocks]))
    if n_used > 6:
        A, out["rank_margin"] = compress_tracked(A)
        out["m"] = A.v.shape[0]
        if out["m"] == 0:
            return out
    Hc = V(A.v[:, :12], A.e[:, :12]); rc = V(A.v[:, 12], A.e[:, 12])
    t = F.update_tracked(P, cols, Hc, rc, np.eye(Hc.v.shape[0]), 0.0)
    out.update(batch_status=t["status"], pmin=t["pmin"], H=Hc, r=rc)
    if t["status"] == 0:
        out.update(gamma_b=t["gamma"], e_gamma_b=t["e_gamma"], dx=t["dx"], e_dx=t["e_dx"], P=t["P"], e_P=t["e_P"])
    return out


def batch_plain(P, job, obs, mutate=None, status=None, drop_extrinsics=False):
    """the definition, literally: the rows of the used observations uncompressed and unwhitened, R = blockdiag(R_k),
    K = P H^T (H P H^T + R)^-1, dx = K r, P <- P - K H P, in long double -> dict(status, gamma, dx, P).  status: take these per-observation
    decisions instead of gating (the mutations are compared on the true batch's observations)"""
    P = _ld(P); n = P.shape[0]
    cols = columns(job, swap=mutate == "swap_clone")
    Ps = P[np.ix_(cols, cols)]
    no = len(obs); st_out = np.zeros(no, int); gam = np.zeros(no, LD)
    Hs, rs, Rs = [], [], []
    for k in range(no):
        row = obs_rows(job, obs[k], mutate if mutate in ("sign_g", "no_cov") else None)
        if row["status"] == BEHIND:
            st_out[k] = BEHIND
            continue
        H, r, Rk = row["H"].v.copy(), row["r"].v, row["Rk"].v
        if drop_extrinsics:
            H[:, :6] = 0
        Rk = np.array([[Rk[0, 0], Rk[0, 1]], [Rk[0, 1], Rk[1, 1]]], LD)
        S = H @ Ps @ H.T + Rk
        y = F.fsub(F.chol(S), r); gam[k] = y @ y
        st_out[k] = USED if (not job["gate"] > 0 or gam[k] <= job["gate"]) else GATED
        if (status[k] if status is not None else st_out[k]) == USED:
            Hs.append(H); rs.append(r); Rs.append(Rk)
    out = dict(status=st_out, gamma=gam, dx=np.zeros(n, LD), P=P)
    if not Hs:
        return out
    m = 2 * len(Hs)
    Hd = np.zeros((m, n), LD); Hd[:, cols] = np.concatenate(Hs); r = np.concatenate(rs)
    R = np.zeros((m, m), LD)
    for k, Rk in enumerate(Rs):
        R[2 * k:2 * k + 2, 2 * k:2 * k + 2] = Rk
    S = Hd @ P @ Hd.T + R
    L = F.chol(S)
    W = F.fsub(L, Hd @ P)                       # K = W^T L^-1
    out["dx"] = W.T @ F.fsub(L, r); out["P"] = P - W.T @ W
    return out


# ------------------------------------------------------------------------------------------------ test problems
PAD = 5
_PROBLEMS = None
from larvio_amd.ops import LANDMARK_OBS as OBS_DTYPE        # noqa: E402  (lvk_landmark_obs: the one definition)


def make_obs(rng, job, n_obs, frac_out=0.0, frac_behind=0.0, zero_cov=False):
    """points 1.5 - 10 m in front of the camera inside a 50 degree cone, observed with N(0, sigma^2) noise, sigma 2e-3 .. 1e-2, each with a
    full covariance of sigmas 1e-3 .. 5e-2 m (or none); a fraction moved 0.5 - 1.5 off in the image (gross outliers), a fraction put
    0.2 - 3 m behind the camera"""
    Rb = np.asarray(quat_to_rot(_ld(job["q_b"])), np.float64); Re = job["R_b2c"]
    o = np.zeros(n_obs, OBS_DTYPE)
    kind = rng.uniform(0, 1, n_obs)
    for k in range(n_obs):
        z = rng.uniform(1.5, 10.0); uv = rng.uniform(-0.45, 0.45, 2)
        if kind[k] < frac_behind:
            z = -rng.uniform(0.2, 3.0)
        pc = np.array([uv[0] * z, uv[1] * z, z])
        o[k]["p_w"] = job["p_b"] + Rb @ (Re.T @ pc + job["t_c_b"])
        o[k]["sigma"] = rng.uniform(2e-3, 1e-2)
        o[k]["uv"] = uv + rng.normal(0, o[k]["sigma"], 2)
        if frac_behind <= kind[k] < frac_behind + frac_out:
            o[k]["uv"] += rng.choice([-1, 1], 2) * rng.uniform(0.5, 1.5, 2)
        if not zero_cov and k % 7 != 3:                                  # (every seventh point is exactly known)
            o[k]["cov_w"] = F._spd(rng, 3, 1e-3, 5e-2).ravel()
    return o


def make_problem(name, seed, n, ldp, n_clones, rank, n_obs, gate=0.0, frac_out=0.0, frac_behind=0.0, zero_cov=False, no_extrinsics=False, leg=22, shift=None):
    """P = D C D with variances log-uniform over 1e-8 .. 1 plus a gauge component of variance 1e2 over the IMU pose and every clone
    (pose_rel_ref's recipe); the clone `rank` of n_clones carries the batch.  no_extrinsics: rows and columns 15..20 of P zero."""
    rng = np.random.default_rng([20261021, seed])
    imu = random_slot(rng, 0, 6)
    clones = [random_slot(rng, leg + 6 * c, leg + 6 * c + 3) for c in range(n_clones)]
    P = with_gauge(filter_like_cov(rng, n), [imu] + clones)
    if no_extrinsics:
        P[15:21, :] = 0; P[:, 15:21] = 0
    qe = rng.normal(0, 1, 4); qe /= np.linalg.norm(qe)
    c = clones[rank]
    job = make_job(c[0], c[2], c[3], np.asarray(quat_to_rot(_ld(qe)), np.float64), rng.uniform(-0.1, 0.1, 3), gate=gate)
    obs = make_obs(rng, job, n_obs, frac_out, frac_behind, zero_cov)
    return dict(name=name, n=n, ldp=ldp, P=P, job=job, obs=obs, mixed=frac_out > 0 or frac_behind > 0, zero_cov=zero_cov)


def stage_problems():
    """Every problem the GPU stage tests run, built once: n_obs = 1, 5, 6, 7, 63, 64, 65, 256, 257 and 1024; n = 28 (clone_col 22: the
    last six columns), 216 and 433, ldp = n and n + PAD; the clone first, in the middle and last in the window; batches with gross
    outliers and points behind the camera under the filter's own gate and under the 99.9 % gate."""
    global _PROBLEMS
    if _PROBLEMS is not None:
        return _PROBLEMS
    g5, g999 = CHI2_005_2, GATE_999 * CHI2_005_2
    _PROBLEMS = [
        make_problem("n28 1 obs", 1, 28, 28, 1, 0, 1),
        make_problem("n28 5 obs", 2, 28, 28 + PAD, 1, 0, 5, gate=g999),
        make_problem("n28 6 obs", 3, 28, 28, 1, 0, 6, zero_cov=True),
        make_problem("n28 7 obs", 4, 28, 28 + PAD, 1, 0, 7),
        make_problem("n216 63 first", 5, 216, 216, 32, 0, 63, gate=g999),
        make_problem("n216 64 middle", 6, 216, 216 + PAD, 32, 15, 64),
        make_problem("n216 65 last", 7, 216, 216, 32, 31, 65, no_extrinsics=True),
        make_problem("n216 mixed 40", 8, 216, 216 + PAD, 32, 7, 40, gate=g5, frac_out=0.3, frac_behind=0.2),
        make_problem("n433 256 middle", 9, 433, 433 + PAD, 68, 30, 256),
        make_problem("n433 257 last", 10, 433, 433, 68, 67, 257, gate=g999),
        make_problem("n433 1024 first", 11, 433, 433 + PAD, 68, 0, 1024),
        make_problem("n433 mixed 300", 12, 433, 433, 68, 40, 300, gate=g999, frac_out=0.3, frac_behind=0.1),
        make_problem("n28 mixed 9", 13, 28, 28, 1, 0, 9, gate=g5, frac_out=0.4, frac_behind=0.2),
    ]
    return _PROBLEMS


_TRACKED = None


def stage_tracked():
    """[(problem, batch_tracked(problem))] of every stage problem, computed once per process"""
    global _TRACKED
    if _TRACKED is None:
        _TRACKED = [(pr, batch_tracked(pr["P"], pr["job"], pr["obs"])) for pr in stage_problems()]
    return _TRACKED


def job_record(job, **kw):
    """the stage entry's job record"""
    from larvio_amd.ops import LANDMARK_FIX_JOB
    j = np.zeros(1, LANDMARK_FIX_JOB)
    for k in ("clone_col", "q_b", "p_b", "t_c_b", "gate", "min_depth"):
        j[k] = job[k]
    j["R_b2c"] = job["R_b2c"].ravel()
    for k, v in kw.items():
        j[k] = v
    return j


def worst_ratio(diff, bound):
    return F.worst_ratio(diff, bound)
