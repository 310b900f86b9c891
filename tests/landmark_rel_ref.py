"""Long-double restatement of what lvk_ekf_landmark_rel_cov (include/lvk_c.h) defines: an anchored inverse-depth landmark in the camera
frame of a target pose b,
    p_w = R_c2w [u v 1] / rho + p_a + R_a t_c_b   (R_c2w = R_a R_b2c^T through a quaternion and back, as lvk_ekf_landmark_cov takes it),
    p_c = R_b2c (R_b^T (p_w - p_b) - t_c_b),
and Sigma = J P_s J^T, P_s = P over the columns [d_theta_e d_t | d_theta_a d_p_a | d_theta_b | d_p_b | d_rho].

Two routes to Sigma:
  * jacobian_nd(): central differences of p_c under the filter's state injection (attitudes q <- small_angle_quat(d_theta) * q,
    positions p <- p + d_p, R_b2c <- R_b2c R(small_angle_quat(d_theta_e))^T, t_c_b <- t_c_b + d_t, rho <- rho + d_rho), written from
    the geometry.  No derivative is written down on that route.
  * the closed form (jacobian_closed(), and tracked(), which carries it through a first-order running error analysis of the float64
    operations the kernel performs: class V of tests/msckf_point_ref.py).  tests/test_landmark_rel_ref.py holds the two routes to each
    other.
The GPU tests compare the kernel with the closed-form route's long-double value inside the derived bound; the central-difference route
ties that value to the geometry.

A pose slot is (theta_col, p_col, q, p) as in tests/pose_rel_ref.py.  A job is dict(a=anchor slot (p_col = theta_col + 3), b=target slot
(a is b: the target is the anchor clone), feat_col, R_b2c (3 x 3), t_c_b, obs (u, v), rho)."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, rot_to_quat, quat_mul, small_angle_quat, skew
from tests.msckf_point_ref import V, mm, stack, skew_v, LD, U, U_LD
from tests.pose_rel_ref import gauge_matrix, filter_like_cov, with_gauge, random_slot, buffer, GAUGE_VAR, PAD      # noqa: F401

N_ERR = 19
H_STEP = LD(2.0) ** -21           # central-difference step, as landmark_cov_ref.H_STEP
# The closed-form J against the central-difference J, entrywise, relative to s = 1 + |f_A| + |g| + |t_c_b| (the size of the function
# differentiated and of its arguments; d p_c / d rho is |f_A| / rho, relative to s / rho).  Truncation: h^2 f''' / 6 = 3.8e-14 f''' with
# f''' <= a few s for the rotations (every derivative of a rotation keeps its norm) and 6 s / rho^3 for rho, i.e. 2.3e-13 (h / rho)^2
# relative to s / rho: at the shallowest rho the problems use (1 / 30 m) h / rho = 1.4e-5, nothing.  Rounding: ~150 long-double
# operations on numbers of size s, 150 * 2^-64 s, divided by 2 h = 9.5e-7: 8.5e-12 s.  1e-10 leaves a factor 10.
TOL_ND = 1e-10


def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ the geometry
def point_in_camera(job, delta=None):
    """p_c after the injection of delta (19 components in the order of the gathered columns; zero when None).  With the target the anchor
    clone itself (a is b) the one pose takes the anchor's and the target's components together."""
    d = np.zeros(N_ERR, LD) if delta is None else np.asarray(delta, LD)
    a, b = job["a"], job["b"]
    da, db = d[6:12], np.concatenate([d[12:15], d[15:18]])
    if a is b:
        da = db = da + db
    q_a = quat_mul(small_angle_quat(da[0:3]), _ld(a[2])); p_a = _ld(a[3]) + da[3:6]
    q_b = quat_mul(small_angle_quat(db[0:3]), _ld(b[2])); p_b = _ld(b[3]) + db[3:6]
    R_b2c = _ld(job["R_b2c"]).reshape(3, 3) @ quat_to_rot(small_angle_quat(d[0:3])).T
    t_c_b = _ld(job["t_c_b"]) + d[3:6]
    rho = LD(job["rho"]) + d[18]
    R_a = quat_to_rot(q_a)
    R_c2w = quat_to_rot(rot_to_quat(R_a @ R_b2c.T))
    u, v = _ld(job["obs"])
    p_w = R_c2w @ np.array([u / rho, v / rho, 1 / rho], LD) + p_a + R_a @ t_c_b
    return R_b2c @ (quat_to_rot(q_b).T @ (p_w - p_b) - t_c_b)


def jacobian_nd(job, h=H_STEP):
    """3 x 19, central differences of point_in_camera at step h.  a is b: the pose moves as one, so columns 6..11 and 12..17 each hold
    the derivative along the common pose; use merged() before comparing or contracting"""
    J = np.zeros((3, N_ERR), LD)
    for k in range(N_ERR):
        d = np.zeros(N_ERR, LD); d[k] = h
        J[:, k] = (point_in_camera(job, d) - point_in_camera(job, -d)) / (2 * h)
    return J


def merged(job, J, nd):
    """J with the target's six columns folded into the anchor's when a is b (P_s then holds the same columns twice, and J P_s J^T only
    sees the sum of the two blocks).  nd: J comes from jacobian_nd, whose two blocks each ARE that sum already"""
    if job["a"] is not job["b"]:
        return J
    J = J.copy()
    if not nd:
        J[:, 6:12] += J[:, 12:18]
    J[:, 12:18] = 0
    return J


def geometry(job):
    """long double: (R_a, R_b, R_e, M, f_A, r_c, r, g, y, p_c) of the definition"""
    a, b = job["a"], job["b"]
    R_a = quat_to_rot(_ld(a[2])); R_b = quat_to_rot(_ld(b[2])); R_e = _ld(job["R_b2c"]).reshape(3, 3); t = _ld(job["t_c_b"])
    rho = LD(job["rho"]); u, v = _ld(job["obs"])
    f_A = np.array([u / rho, v / rho, 1 / rho], LD)
    r_c = quat_to_rot(rot_to_quat(R_a @ R_e.T)) @ f_A
    r = r_c + R_a @ t
    g = r + (_ld(a[3]) - _ld(b[3]))
    M = R_e @ R_b.T
    y = R_b.T @ g - t
    return R_a, R_b, R_e, M, f_A, r_c, r, g, y, R_e @ y


def jacobian_closed(job, mutate=None):
    """J = [R_e [y]x - M [r_c]x R_a | M R_a - R_e | -M [r]x | M | M [g]x | -M | -M r_c / rho], long double ([r_c]x R_a = R_a [x]x with
    x = R_e^T f_A).  mutate: None, "sign" (the M [g]x block negated) or "swap" (the anchor's and the target's blocks exchanged, the columns
    staying where they are)"""
    R_a, R_b, R_e, M, f_A, r_c, r, g, y, _ = geometry(job)
    Jg = M @ skew(g)
    if mutate == "sign":
        Jg = -Jg
    blocks = [R_e @ skew(y) - M @ skew(r_c) @ R_a, M @ R_a - R_e, -M @ skew(r), M, Jg, -M, (-(M @ r_c) / LD(job["rho"])).reshape(3, 1)]
    if mutate == "swap":
        blocks = blocks[:2] + [blocks[4], blocks[5], blocks[2], blocks[3]] + blocks[6:]
    return np.concatenate(blocks, axis=1)


def columns(job, plus3=False):
    """the 19 columns of P a job reads; plus3: the mutation that takes the target's position columns as theta + 3"""
    a, b = job["a"], job["b"]
    bp = b[0] + 3 if plus3 else b[1]
    return np.array([15, 16, 17, 18, 19, 20] + [a[0] + k for k in range(6)] + [b[0], b[0] + 1, b[0] + 2, bp, bp + 1, bp + 2, int(job["feat_col"])])


def gather(P, job, plus3=False):
    c = columns(job, plus3)
    return np.asarray(P, np.float64)[np.ix_(c, c)].astype(LD)


def sigma(job, P, mutate=None):
    """Sigma in long double by the closed form, plainly (mutate: see jacobian_closed; "plus3": see columns)"""
    J = jacobian_closed(job, mutate if mutate in ("sign", "swap") else None)
    return J @ gather(P, job, plus3=mutate == "plus3") @ J.T


def sigma_nd(job, P):
    J = merged(job, jacobian_nd(job), nd=True)
    return J @ gather(P, job) @ J.T


# ------------------------------------------------------------------------------------------------ running error analysis
def _sqrt_v(x):
    v = np.sqrt(x.v)
    return V(v, x.e / (2 * v) + U * np.abs(v))


def _q2r_v(x, y, z, w):
    tx, ty, tz = x * 2, y * 2, z * 2
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = V(LD(1))
    return stack([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]])


def _r2q_v(m):
    """Eigen's Quaternion(Matrix3) on tracked entries -> (x, y, z, w); the branch is the one the values take"""
    e = lambda i, j: m[i][j]
    t = e(0, 0) + e(1, 1) + e(2, 2)
    half = V(LD(0.5))
    if t.v > 0:
        t = _sqrt_v(t + V(LD(1)))
        w = half * t
        t = half / t
        return (e(2, 1) - e(1, 2)) * t, (e(0, 2) - e(2, 0)) * t, (e(1, 0) - e(0, 1)) * t, w
    i = 0
    if m.v[1, 1] > m.v[0, 0]:
        i = 1
    if m.v[2, 2] > m.v[i, i]:
        i = 2
    j = (i + 1) % 3; k = (j + 1) % 3
    t = _sqrt_v(e(i, i) - e(j, j) - e(k, k) + V(LD(1)))
    q = [None] * 3
    q[i] = half * t
    t = half / t
    w = (e(k, j) - e(j, k)) * t
    q[j] = (e(j, i) + e(i, j)) * t
    q[k] = (e(k, i) + e(i, k)) * t
    return q[0], q[1], q[2], w


def _hcat(blocks):
    return V(np.concatenate([b.v for b in blocks], axis=1), np.concatenate([b.e for b in blocks], axis=1))


def tracked(job, P):
    """-> (p_c, err_p, Sigma, err, Bnd): the long-double p_c and Sigma of the closed-form route, the derived componentwise bounds on the
    float64 kernel's errors against them and the entrywise scale Bnd = |J| |P_s| |J|^T.

    The bound is first order in u = 2^-53 and follows the kernel (be_landmark_rel.hip) operation by operation (class V): the nine
    entries of R(q_anchor) and R(q_b) (3 - 4 roundings each); R_a R_e^T, its quaternion (a square root, a division, three differences and
    products) and the matrix of that quaternion; f_A (three divisions); r_c, R_a t_c_b, M = R_e R_b^T, R_b^T g, p_c = R_e y and every
    3 x 3 product of J's blocks as inner products of length 3 (gamma_3 |.| |.|); the sums and differences r, p_a - p_b, g, y,
    R_e [y]x + M A_e, M R_a - R_e (one rounding each); -M r_c / rho (a division); T = J P_s and T J^T as inner products of length 19
    summed in order (gamma_19 |J| |P_s| and gamma_19 |T| |J^T|, on top of what the operands carry).  The whole is doubled for the terms of
    higher order, and this file's own rounding (u_ld / u of the same expression, and u_ld per term of the scale) is added.  Nothing in
    it is fitted to a result."""
    a, b = job["a"], job["b"]
    qa = [V(c) for c in _ld(a[2])]; qb = [V(c) for c in _ld(b[2])]
    Ra = _q2r_v(*qa); Rb = _q2r_v(*qb)
    Re = V(_ld(job["R_b2c"]).reshape(3, 3)); te = V(_ld(job["t_c_b"]))
    Rc = _q2r_v(*_r2q_v(mm(Ra, Re.T)))
    rho = V(LD(job["rho"])); u, v = (V(c) for c in _ld(job["obs"]))
    fa = stack([u / rho, v / rho, V(LD(1)) / rho])
    rc = mm(Rc, fa)
    r = rc + mm(Ra, te)
    g = r + (V(_ld(a[3])) - V(_ld(b[3])))
    M = mm(Re, Rb.T)
    y = mm(Rb.T, g) - te
    pc = mm(Re, y)
    Ae = mm(-skew_v(rc), Ra)
    last = -(mm(M, rc) / rho)
    J = _hcat([mm(Re, skew_v(y)) + mm(M, Ae), mm(M, Ra) - Re, mm(M, -skew_v(r)), M, mm(M, skew_v(g)), -M, V(last.v.reshape(3, 1), last.e.reshape(3, 1))])
    Ps = gather(P, job)
    S = mm(mm(J, V(Ps)), J.T)
    Bnd = np.abs(J.v) @ np.abs(Ps) @ np.abs(J.v).T
    err = np.triu(S.e) + np.triu(S.e, 1).T                      # the kernel computes the upper triangle and copies it
    err = 2 * err * (1 + U_LD / U) + U_LD * Bnd * 2 * N_ERR
    scale_p = np.abs(Re.v) @ (np.abs(Rb.v.T) @ np.abs(g.v) + np.abs(te.v))
    err_p = 2 * pc.e * (1 + U_LD / U) + U_LD * scale_p * 8
    return pc.v, err_p, S.v, err, Bnd


# ------------------------------------------------------------------------------------------------ test problems
def random_extrinsics(rng):
    """a camera rotated and offset from the body like a real rig, as landmark_cov_ref.random_job draws it"""
    qe = rng.normal(0, 1, 4); qe /= np.linalg.norm(qe)
    return np.asarray(quat_to_rot(qe), np.float64), rng.normal(0, 0.1, 3)


def random_point(rng, a, b, feat_col, R_b2c, t_c_b):
    """a bearing inside a 90 degree field of view, depth (metres along the anchor's optical axis) log-uniform over 0.3 .. 30"""
    return dict(a=a, b=b, feat_col=int(feat_col), R_b2c=R_b2c, t_c_b=t_c_b, obs=rng.uniform(-1, 1, 2), rho=float(1.0 / 10.0 ** rng.uniform(np.log10(0.3), np.log10(30.0))))


def make_launch(name, seed, leg, n_clones, n, ldp, pick):
    """slots: the IMU state (columns 0 / 6, split) and every clone (leg + 6 c / + 3), positions inside a ball of 5 m, arbitrary attitudes;
    the feature columns are leg + 6 n_clones .. n - 1.  P = D C D with variances log-uniform over 1e-8 .. 1, plus the gauge component
    (a world rotation about z and a translation, variance 1e2, over every pose slot).  pick(rng, imu, clones, feats, point) -> jobs"""
    rng = np.random.default_rng([20261020, seed])
    imu = random_slot(rng, 0, 6)
    clones = [random_slot(rng, leg + 6 * c, leg + 6 * c + 3) for c in range(n_clones)]
    feats = list(range(leg + 6 * n_clones, n))
    R_b2c, t_c_b = random_extrinsics(rng)
    slots = [imu] + clones
    P = with_gauge(filter_like_cov(rng, n), slots)
    point = lambda a, b, fc: random_point(rng, a, b, fc, R_b2c, t_c_b)
    return dict(name=name, n=n, ldp=ldp, P=P, slots=slots, jobs=pick(rng, imu, clones, feats, point))


_LAUNCHES = None


def stage_launches():
    """Every launch the GPU stage tests make against the restatement, built once: n = 29 (22 + one clone + one feature) with the target
    the anchor clone and with the target the IMU state; n = 58 (46 + one clone + six features) with a padded ldp and the feature in the
    last column; n = 60 (46 + 12 + 2); n = 433 (22 + 62 clones + 39 features) with 1, 65 and 300 jobs."""
    global _LAUNCHES
    if _LAUNCHES is not None:
        return _LAUNCHES
    out = [
        make_launch("n29 b = a", 1, 22, 1, 29, 29, lambda r, imu, cl, ft, pt: [pt(cl[0], cl[0], ft[0])]),
        make_launch("n29 b = imu", 2, 22, 1, 29, 29, lambda r, imu, cl, ft, pt: [pt(cl[0], imu, ft[0])]),
        make_launch("n58 padded", 3, 46, 1, 58, 58 + PAD, lambda r, imu, cl, ft, pt: [pt(cl[0], imu, ft[-1]), pt(cl[0], cl[0], ft[-1]), pt(cl[0], imu, ft[0])]),
        make_launch("n60", 4, 46, 2, 60, 60, lambda r, imu, cl, ft, pt: [pt(cl[0], cl[1], ft[0]), pt(cl[1], cl[0], ft[1]), pt(cl[1], imu, ft[1]), pt(cl[1], cl[1], ft[0])]),
        make_launch("n433 1 job", 5, 22, 62, 433, 433, lambda r, imu, cl, ft, pt: [pt(cl[61], cl[0], ft[-1])]),
    ]

    def many(count):
        def pick(r, imu, cl, ft, pt):
            jobs = []
            for k in range(count):
                a = cl[int(r.integers(0, len(cl)))]
                b = imu if k % 3 == 0 else a if k % 7 == 1 else cl[int(r.integers(0, len(cl)))]
                jobs.append(pt(a, b, ft[int(r.integers(0, len(ft)))]))
            return jobs
        return pick
    out.append(make_launch("n433 65", 6, 22, 62, 433, 433 + PAD, many(65)))
    out.append(make_launch("n433 300", 7, 22, 62, 433, 433, many(300)))
    _LAUNCHES = out
    return out


def pack(jobs):
    """the stage entry's job records"""
    from larvio_amd.ops import LANDMARK_REL_JOB
    rec = np.zeros(len(jobs), LANDMARK_REL_JOB)
    for k, j in enumerate(jobs):
        a, b = j["a"], j["b"]
        rec[k]["anchor_col"] = a[0]; rec[k]["feat_col"] = j["feat_col"]; rec[k]["q_anchor"] = a[2]; rec[k]["p_anchor"] = a[3]
        rec[k]["R_b2c"] = np.asarray(j["R_b2c"], np.float64).reshape(9); rec[k]["t_c_b"] = j["t_c_b"]; rec[k]["obs_anchor"] = j["obs"]; rec[k]["inv_depth"] = j["rho"]
        rec[k]["b_theta_col"] = b[0]; rec[k]["b_p_col"] = b[1]; rec[k]["q_b"] = b[2]; rec[k]["p_b"] = b[3]
    return rec


def unpack(rec):
    """job dicts from LANDMARK_REL_JOB records (a target that names the anchor's columns is the anchor slot itself)"""
    jobs = []
    for r in np.atleast_1d(rec):
        a = (int(r["anchor_col"]), int(r["anchor_col"]) + 3, np.array(r["q_anchor"]), np.array(r["p_anchor"]))
        same = int(r["b_theta_col"]) == a[0] and int(r["b_p_col"]) == a[1]
        b = a if same else (int(r["b_theta_col"]), int(r["b_p_col"]), np.array(r["q_b"]), np.array(r["p_b"]))
        jobs.append(dict(a=a, b=b, feat_col=int(r["feat_col"]), R_b2c=np.array(r["R_b2c"]).reshape(3, 3), t_c_b=np.array(r["t_c_b"]), obs=np.array(r["obs_anchor"]),
                         rho=float(r["inv_depth"])))
    return jobs


# ------------------------------------------------------------------------------------------------ the filter's map
CHI2_3_999 = 16.27            # the 99.9 % quantile of chi-square with 3 degrees of freedom


def filter_jobs(state, clones, ids, idp, pos, anchor_ids=None, obs=None, to_clone_id=-1, leg=22):
    """The jobs lvk_ekf_get_feature_rel builds, from what the getters hand out: state (dict of lvk_ekf_get_state), clones, the in-state
    features (ids, inverse depths, world positions).  anchor_ids None (the oracle's filter does not hand them out): the anchor is the
    clone along whose optical axis the point's depth is 1 / rho (to 1e-9; no such clone: the feature is skipped); obs None: the anchor
    observation is recovered from the position.  -> (jobs, rows): rows = the features' indices"""
    if to_clone_id == -1:
        b = (0, 6, np.array(state["q"], np.float64), np.array(state["p"], np.float64))
    else:
        k = int(np.flatnonzero(clones["id"] == to_clone_id)[0])
        b = (leg + 6 * k, leg + 6 * k + 3, np.array(clones["q"][k]), np.array(clones["p"][k]))
    jobs, rows = [], []
    for i in range(len(ids)):
        cand = range(len(clones)) if anchor_ids is None else np.flatnonzero(clones["id"] == anchor_ids[i])
        best = None
        for k in cand:
            f = np.linalg.solve(np.asarray(quat_to_rot(np.asarray(clones["q_cam"][k], np.float64)), np.float64), pos[i] - clones["p_cam"][k])
            miss = abs(1.0 / f[2] - idp[i]) / abs(idp[i])
            if best is None or miss < best[0]:
                best = (miss, int(k), f)
        if best is None or (anchor_ids is None and best[0] > 1e-9):
            continue
        _, k, f = best
        a = (leg + 6 * k, leg + 6 * k + 3, np.array(clones["q"][k]), np.array(clones["p"][k]))
        if b[0] == a[0]:
            b_k = a
        else:
            b_k = b
        jobs.append(dict(a=a, b=b_k, feat_col=leg + 6 * len(clones) + i, R_b2c=np.array(state["R_b2c"], np.float64).reshape(3, 3), t_c_b=np.array(state["t_c_b"], np.float64),
                         obs=np.array([f[0] / f[2], f[1] / f[2]]) if obs is None else np.asarray(obs[i], np.float64), rho=float(idp[i])))
        rows.append(i)
    return jobs, rows
