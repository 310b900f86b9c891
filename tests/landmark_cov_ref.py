"""Long-double restatement of what lvk_ekf_landmark_cov (include/lvk_c.h) defines: the filter's state injection applied to the
thirteen error components a landmark's position depends on, the position formula of the anchored inverse-depth parametrisation, and
Sigma = J P_s J^T with J taken by central differences of that composition - no derivative is written down here.

Conventions are those of larvio_amd/csrc/be_host_math.h (Hamilton quaternions [x y z w], Eigen's quaternion <-> matrix formulas);
tests/test_landmark_cov_ref.py holds the helpers below to that header compiled on the host, and the composition to closed forms.

The error vector is ordered as the gathered columns of P: [d_theta_e(3) d_t(3) | d_theta(3) d_p(3) | d_rho]."""
import numpy as np

LD = np.longdouble
N_ERR = 13
H_STEP = LD(2.0) ** -21           # central-difference step: truncation ~ h^2 f'''/6 and rounding ~ 2^-64 / h meet near 2^-21
# 10 x the largest |Sigma(h) - Sigma(h/2)| / B over test_landmark_cov_ref.py::test_differentiation_error_sets_tol_nd's cases
# (landmarks 0.5 - 5 m deep, B = |J| |P_s| |J|^T); measured there on the CPU: 7.4e-12
TOL_ND = 7.4e-11


def quat_to_rot(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype=np.result_type(x))


def rot_to_quat(m):
    q = np.zeros(4, m.dtype)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1)
        q[3] = t / 2
        t = 1 / (2 * t)
        q[0] = (m[2, 1] - m[1, 2]) * t; q[1] = (m[0, 2] - m[2, 0]) * t; q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1)
        q[i] = t / 2
        t = 1 / (2 * t)
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], dtype=np.result_type(ax, bx))


def small_angle_quat(dtheta):
    d = np.asarray(dtheta) / 2
    n2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    if n2 <= 1:
        return np.array([d[0], d[1], d[2], np.sqrt(1 - n2)], dtype=d.dtype)
    s = np.sqrt(1 + n2)
    return np.array([d[0] / s, d[1] / s, d[2] / s, 1 / s], dtype=d.dtype)


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.asarray(w).dtype)


def _ld(job, key):
    return np.asarray(job[key], np.float64).astype(LD)


def poses(job, delta=None, p_anchor=None):
    """the injected state a landmark's position is computed from: (p_clone, p_cam, R_c2w, rho), long double.  The steps are inject()'s
    and clone_refresh_cam's (backend.hip): the clone's camera attitude goes through a quaternion and back."""
    d = np.zeros(N_ERR, LD) if delta is None else np.asarray(delta, LD)
    q = quat_mul(small_angle_quat(d[6:9]), _ld(job, "q_anchor"))
    p = (np.zeros(3, LD) if p_anchor is None else np.asarray(p_anchor, LD)) + d[9:12]
    R_b2c = _ld(job, "R_b2c").reshape(3, 3) @ quat_to_rot(small_angle_quat(d[0:3])).T
    t_c_b = _ld(job, "t_c_b") + d[3:6]
    rho = LD(job["inv_depth"]) + d[12]
    R_b2w = quat_to_rot(q)
    R_c2w = quat_to_rot(rot_to_quat(R_b2w @ R_b2c.T))
    return p, p + R_b2w @ t_c_b, R_c2w, rho


def position(job, delta=None, p_anchor=None):
    """Feature::position after the injection of delta (13 components, zero when None)"""
    _, p_cam, R_c2w, rho = poses(job, delta, p_anchor)
    u, v = _ld(job, "obs_anchor")
    return R_c2w @ np.array([u / rho, v / rho, 1 / rho], LD) + p_cam


def jacobian_nd(job, h=H_STEP):
    """3 x 13, central differences of position() at step h"""
    J = np.zeros((3, N_ERR), LD)
    for k in range(N_ERR):
        d = np.zeros(N_ERR, LD); d[k] = h
        J[:, k] = (position(job, d) - position(job, -d)) / (2 * h)
    return J


def columns(job):
    a = int(job["anchor_col"])
    return np.array([15, 16, 17, 18, 19, 20, a, a + 1, a + 2, a + 3, a + 4, a + 5, int(job["feat_col"])])


def gather(P, job):
    """the 13 x 13 block of P the job reads, long double"""
    c = columns(job)
    return np.asarray(P, np.float64)[np.ix_(c, c)].astype(LD)


def sigma_from(J, Ps):
    return J @ Ps @ J.T


def bound(J, Ps):
    """B = |J| |P_s| |J|^T, the entrywise scale every comparison is relative to"""
    return np.abs(J) @ np.abs(Ps) @ np.abs(J).T


def sigma(job, P, h=H_STEP):
    """-> (Sigma, B, J) in long double for one job on the covariance P (any array whose [row, col] are P's)"""
    J = jacobian_nd(job, h); Ps = gather(P, job)
    return sigma_from(J, Ps), bound(J, Ps), J


def random_job(rng, anchor_col, feat_col, depth=None):
    """one LANDMARK_JOB record (larvio_amd.ops): random unit attitude, a camera rotated and offset from the body like a real rig, a
    bearing inside a 90 degree field of view, depth (metres along the optical axis) uniform in 0.5 .. 5 unless given"""
    from larvio_amd.ops import LANDMARK_JOB
    j = np.zeros((), LANDMARK_JOB)
    q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
    qe = rng.normal(0, 1, 4); qe /= np.linalg.norm(qe)
    j["anchor_col"] = anchor_col; j["feat_col"] = feat_col
    j["q_anchor"] = q; j["R_b2c"] = quat_to_rot(qe).reshape(9); j["t_c_b"] = rng.normal(0, 0.1, 3)
    j["obs_anchor"] = rng.uniform(-1, 1, 2); j["inv_depth"] = 1.0 / (rng.uniform(0.5, 5.0) if depth is None else depth)
    return j


def random_spd(rng, n, scale=1e-3):
    A = rng.normal(0, 1, (n, n))
    return scale * (A @ A.T) / n + np.diag(rng.uniform(1e-8, 1e-4, n))


def sigma_closed(job, s2):
    """Sigma for P_s = diag(s2[0] I3, s2[1] I3, s2[2] I3, s2[3] I3, s2[4]) (extrinsic rotation, extrinsic translation, anchor attitude,
    anchor position, rho) as the sum of the closed forms test_landmark_cov_ref.py holds the composition to - no differentiation,
    exact to long-double rounding"""
    p_clone, p_cam, _, rho = poses(job)
    p_w = position(job)
    r, r_c = p_w - p_clone, p_w - p_cam
    s2 = np.asarray(s2, LD); I = np.eye(3, dtype=LD)
    return (s2[0] * skew(r_c) @ skew(r_c).T + s2[1] * I + s2[2] * skew(r) @ skew(r).T + s2[3] * I + s2[4] * np.outer(r_c / rho, r_c / rho))
