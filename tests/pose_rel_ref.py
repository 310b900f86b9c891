"""Long-double restatement of what lvk_ekf_pose_rel_cov (include/lvk_c.h) defines: for two poses a, b with
    R_ab = R_a^T R_b,   p_ab = R_a^T (p_b - p_a),
and the error of the relative pose defined by R_ab,true = (I + [d_phi]x) R_ab, p_ab,true = p_ab + d_rho,
    Sigma_rel = J P_s J^T,   P_s = P over the columns [d_theta_a d_p_a d_theta_b d_p_b],   output order [d_phi; d_rho].

Two routes to J:
  * jacobian_nd(): central differences of (log(R_ab' R_ab^T)v, p_ab' - p_ab) under the filter's state injection (attitude
    q <- small_angle_quat(d_theta) * q, position p <- p + d_p), written from the geometry.  No derivative is written down on that route.
  * the closed form (jacobian_closed(), and sigma_tracked(), which carries it through a first-order running error analysis of the
    float64 operations the kernel performs: class V of tests/msckf_point_ref.py).  tests/test_pose_rel_ref.py holds the two routes to
    each other.
The GPU tests compare the kernel with the closed-form route's long-double value inside the derived bound; the central-difference route
ties that value to the geometry.

A pose slot is (theta_col, p_col, q, p): the first of its three attitude columns, the first of its three position columns, its
attitude [x y z w] (body to world) and position.  A job is dict(a=slot or None, b=slot); a None: an absolute job."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, quat_mul, small_angle_quat, skew
from tests.msckf_point_ref import V, mm, quat_to_rot_v, skew_v, LD, U, U_LD

H_STEP = LD(2.0) ** -21           # central-difference step, as landmark_cov_ref.H_STEP
# The closed-form J against the central-difference J, entrywise, relative to (1 + |d|) (the size of the functions differentiated:
# rotations of norm 1 and p_ab of norm |d|).  Truncation: h^2 f''' / 6 = 3.8e-14 f''', f''' <= a few (1 + |d|) (every derivative of a
# rotation keeps its norm; small_angle_quat's angle is |x| + |x|^3 / 24).  Rounding: ~50 long-double operations, 50 * 2^-64 (1 + |d|),
# divided by 2 h = 9.5e-7: 3e-12 (1 + |d|).  1e-10 leaves a factor 30.
TOL_ND = 1e-10


def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


# ------------------------------------------------------------------------------------------------ the geometry
def inject(q, p, d6):
    """the filter's state injection on one pose: d6 = [d_theta d_p]"""
    d6 = np.asarray(d6, LD)
    return quat_mul(small_angle_quat(d6[0:3]), np.asarray(q, LD)), np.asarray(p, LD) + d6[3:6]


def rel_pose(qa, pa, qb, pb):
    """(R_ab, p_ab)"""
    Ra = quat_to_rot(np.asarray(qa, LD))
    return Ra.T @ quat_to_rot(np.asarray(qb, LD)), Ra.T @ (np.asarray(pb, LD) - np.asarray(pa, LD))


def log_so3(R):
    """the rotation vector of a rotation matrix close to the identity"""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD) / 2      # sin(angle) * axis
    s = np.sqrt(w @ w)
    if s < LD(1e-9):
        return w * (1 + s * s / 6)
    return w * (np.arcsin(s) / s)


def rel_error(qa, pa, qb, pb, qa0, pa0, qb0, pb0):
    """[d_phi; d_rho] of the relative pose of (a, b) against that of (a0, b0): R_ab = (I + [d_phi]x) R_ab0 to first order"""
    R1, t1 = rel_pose(qa, pa, qb, pb); R0, t0 = rel_pose(qa0, pa0, qb0, pb0)
    return np.concatenate([log_so3(R1 @ R0.T), t1 - t0])


def jacobian_nd(a, b, h=H_STEP):
    """6 x 12, central differences of the relative pose's error under the injection of [d_theta_a d_p_a d_theta_b d_p_b]; a is b
    (the same slot) moves both ends together"""
    same = a is b
    J = np.zeros((6, 12), LD)
    for k in range(12):
        col = []
        for sgn in (1, -1):
            d = np.zeros(12, LD); d[k] = sgn * h
            da, db = d[0:6], d[6:12]
            if same:
                da = db = d[0:6] + d[6:12]
            qa, pa = inject(a[2], a[3], da); qb, pb = inject(b[2], b[3], db)
            col.append(rel_error(qa, pa, qb, pb, a[2], a[3], b[2], b[3]))
        J[:, k] = (col[0] - col[1]) / (2 * h)
    return J


def jacobian_closed(a, b, mutate=None):
    """J = [-R_a^T 0 R_a^T 0; R_a^T [d]x  -R_a^T  0  R_a^T], long double.  mutate: None, "sign" (the [d]x term negated) or "swap" (J
    built as if a were b and b were a, the columns staying where they are)"""
    if mutate == "swap":
        a, b = b, a
    Rt = quat_to_rot(_ld(a[2])).T
    d = _ld(b[3]) - _ld(a[3])
    Z = np.zeros((3, 3), LD)
    X = Rt @ skew(d)
    if mutate == "sign":
        X = -X
    return np.block([[-Rt, Z, Rt, Z], [X, -Rt, Z, Rt]])


def columns(job, plus3=False):
    """the 12 (absolute: 6) columns of P a job reads; plus3: the mutation that takes every position column as theta + 3"""
    out = []
    for s in ((job["a"], job["b"]) if job["a"] is not None else (job["b"],)):
        out += [s[0], s[0] + 1, s[0] + 2] + ([s[0] + 3, s[0] + 4, s[0] + 5] if plus3 else [s[1], s[1] + 1, s[1] + 2])
    return np.array(out)


def gather(P, job, plus3=False):
    c = columns(job, plus3)
    return np.asarray(P, np.float64)[np.ix_(c, c)].astype(LD)


def sigma(job, P, mutate=None):
    """Sigma_rel in long double by the closed form, plainly (mutate: see jacobian_closed; "plus3": see columns)"""
    J = jacobian_closed(job["a"], job["b"], mutate if mutate in ("sign", "swap") else None)
    return J @ gather(P, job, plus3=mutate == "plus3") @ J.T


def sigma_nd(job, P):
    J = jacobian_nd(job["a"], job["b"])
    return J @ gather(P, job) @ J.T


# ------------------------------------------------------------------------------------------------ running error analysis
def sigma_tracked(job, P):
    """-> (Sigma, err, Bnd): the long-double Sigma_rel of the closed-form route, the derived componentwise bound on the float64
    kernel's error against it and the entrywise scale Bnd = |J| |P_s| |J|^T.

    The bound is first order in u = 2^-53 and follows the kernel operation by operation (class V): the nine entries of R(q_a) (3 - 4
    roundings each); d = p_b - p_a (one each); R_a^T [d]x as inner products of length 3 (gamma_3 |.| |.|); the negations are exact;
    T = J P_s and T J^T as inner products of length 12 summed in order (gamma_12 |.| |.|, on top of what the operands carry).  The
    whole is doubled for the terms of higher order, and this file's own rounding (u_ld / u of the same expression, and u_ld per term
    of Bnd) is added.  Nothing in it is fitted to a result."""
    a, b = job["a"], job["b"]
    R = quat_to_rot_v(a[2])
    d = V(_ld(b[3])) - V(_ld(a[3]))
    Rt = R.T
    X = mm(Rt, skew_v(d))
    Z = np.zeros((3, 3), LD)
    J = V(np.block([[-Rt.v, Z, Rt.v, Z], [X.v, -Rt.v, Z, Rt.v]]), np.block([[Rt.e, Z, Rt.e, Z], [X.e, Rt.e, Z, Rt.e]]))
    Ps = gather(P, job)
    S = mm(mm(J, V(Ps)), J.T)
    Bnd = np.abs(J.v) @ np.abs(Ps) @ np.abs(J.v).T
    err = np.triu(S.e) + np.triu(S.e, 1).T                      # the kernel computes the upper triangle and copies it
    err = 2 * err * (1 + U_LD / U) + U_LD * Bnd * 24
    return S.v, err, Bnd


# ------------------------------------------------------------------------------------------------ test problems
N_GAUGE = 4
GAUGE_VAR = 1e2


def gauge_matrix(slots, n):
    """n x 4: the change of every slot's error components under a rigid motion of the world by a rotation about z and a translation,
    d_theta = theta, d_p = [theta]x p + t = -[p]x theta + t"""
    G = np.zeros((n, N_GAUGE), LD)
    for tc, pc, _, p in slots:
        G[tc + 2, 0] = 1
        G[pc:pc + 3, 0] = -skew(_ld(p))[:, 2]
        G[pc:pc + 3, 1:4] = np.eye(3, dtype=LD)
    return G


def filter_like_cov(rng, n):
    """P = D C D: C a random correlation matrix, D^2 the variances, log-uniform over 1e-8 .. 1"""
    A = rng.normal(0, 1, (n, n + 8))
    C = A @ A.T
    s = 1 / np.sqrt(np.diag(C)); C = C * s[:, None] * s[None, :]
    D = np.sqrt(10.0 ** rng.uniform(-8, 0, n))
    P = C * D[:, None] * D[None, :]
    return (P + P.T) / 2


def with_gauge(P, slots, var=GAUGE_VAR):
    """P + G (var I) G^T, the gauge part formed in long double and rounded once"""
    G = gauge_matrix(slots, P.shape[0])
    return (P.astype(LD) + LD(var) * (G @ G.T)).astype(np.float64)


def random_slot(rng, tc, pc, radius=5.0):
    q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
    v = rng.normal(0, 1, 3); v *= radius * rng.uniform(0, 1) ** (1 / 3) / np.linalg.norm(v)
    return (int(tc), int(pc), q, v)


def make_launch(name, seed, leg, n_clones, n, ldp, pick):
    """slots: the IMU state (columns 0 / 6, split), every clone (leg + 6 c / + 3) and the last six columns of n; positions inside a ball
    of 5 m (|d| up to 10 m), clone 1 - if there is one - at clone 0's position (|d| = 0).  pick(rng, imu, clones, tail) -> jobs"""
    rng = np.random.default_rng([20261019, seed])
    imu = random_slot(rng, 0, 6)
    clones = [random_slot(rng, leg + 6 * c, leg + 6 * c + 3) for c in range(n_clones)]
    if n_clones > 1:
        clones[1] = clones[1][:3] + (clones[0][3].copy(),)
    last = leg + 6 * n_clones == n
    tail = clones[-1] if last else random_slot(rng, n - 6, n - 3)      # b on the last six columns of n
    slots = [imu] + clones + ([] if last else [tail])
    P = with_gauge(filter_like_cov(rng, n), slots)
    return dict(name=name, n=n, ldp=ldp, P=P, slots=slots, jobs=pick(rng, imu, clones, tail))


def rel(a, b):
    return dict(a=a, b=b)


def absolute(b):
    return dict(a=None, b=b)


PAD = 5
_LAUNCHES = None


def stage_launches():
    """Every launch the GPU stage tests make against the restatement, built once: n = 28 (one clone), 46 + 12 and 433 (a 62-clone
    window and three more columns), ldp = n and n + PAD, 1 / 2 / 61 / 300 jobs; a on the IMU state (columns 0 and 6), b on the last
    six columns of n, a == b, |d| = 0, absolute jobs among relative ones."""
    global _LAUNCHES
    if _LAUNCHES is not None:
        return _LAUNCHES
    out = [
        make_launch("n28 1 job", 1, 22, 1, 28, 28, lambda r, imu, cl, tail: [rel(imu, tail)]),
        make_launch("n28 mixed", 2, 22, 1, 28, 28 + PAD, lambda r, imu, cl, tail: [absolute(cl[0]), rel(imu, cl[0]), rel(cl[0], cl[0]), absolute(imu), rel(cl[0], imu)]),
        make_launch("n58 2 jobs", 3, 46, 2, 58, 58, lambda r, imu, cl, tail: [rel(cl[0], cl[1]), rel(cl[1], cl[1])]),
        make_launch("n58 padded", 4, 46, 2, 58, 58 + PAD, lambda r, imu, cl, tail: [rel(imu, tail), absolute(tail), rel(cl[1], cl[0])]),
        make_launch("n433 edges", 5, 22, 62, 433, 433, lambda r, imu, cl, tail: [rel(cl[i], cl[i + 1]) for i in range(61)]),
    ]

    def many(r, imu, cl, tail):
        pool = [imu, tail] + cl
        jobs = []
        for k in range(300):
            i, j = (int(x) for x in r.integers(0, len(pool), 2))
            jobs.append(absolute(pool[j]) if k % 5 == 4 else rel(pool[i], pool[i if k % 37 == 0 else j]))
        return jobs
    out.append(make_launch("n433 300", 6, 22, 62, 433, 433 + PAD, many))
    _LAUNCHES = out
    return out


def pack(jobs):
    """the stage entry's job records"""
    from larvio_amd.ops import POSE_REL_JOB
    rec = np.zeros(len(jobs), POSE_REL_JOB)
    for k, j in enumerate(jobs):
        a, b = j["a"], j["b"]
        rec[k]["b_theta_col"] = b[0]; rec[k]["b_p_col"] = b[1]; rec[k]["q_b"] = b[2]; rec[k]["p_b"] = b[3]
        if a is None:
            rec[k]["a_theta_col"] = -1; rec[k]["a_p_col"] = -1
        else:
            rec[k]["a_theta_col"] = a[0]; rec[k]["a_p_col"] = a[1]; rec[k]["q_a"] = a[2]; rec[k]["p_a"] = a[3]
    return rec


def buffer(P, n, ldp):
    """P in a row-major buffer of leading dimension ldp, NaN in the padding (never read)"""
    b = np.full((n, ldp), np.nan); b[:, :n] = P
    return b


# ------------------------------------------------------------------------------------------------ the filter's window
CHI2_6_999 = 22.46            # the 99.9 % quantile of chi-square with 6 degrees of freedom


def clone_slot(clone, rank, leg=22):
    return (leg + 6 * rank, leg + 6 * rank + 3, np.array(clone["q"], np.float64), np.array(clone["p"], np.float64))


def window_sigma(P, clones, leg=22):
    """Sigma_rel (float64) of every consecutive pair of a clone list on the covariance P"""
    return [sigma(rel(clone_slot(clones[i], i, leg), clone_slot(clones[i + 1], i + 1, leg)), P).astype(np.float64) for i in range(len(clones) - 1)]


def true_pose(traj, t):
    from larvio_amd.synthetic import R2q
    return R2q(traj.R_wb(t)), traj.p_wb(t)


def edge_d2(traj, ta, tb, qa, pa, qb, pb, S):
    """d2 = e^T Sigma^-1 e of the estimated relative pose of (a, b) against the trajectory's at the two times"""
    qa0, pa0 = true_pose(traj, ta); qb0, pb0 = true_pose(traj, tb)
    e = rel_error(qa0, pa0, qb0, pb0, qa, pa, qb, pb).astype(np.float64)
    return float(e @ np.linalg.solve(S, e))
