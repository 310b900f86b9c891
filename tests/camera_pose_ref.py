"""Long-double restatement of what lvk_ekf_camera_pose_cov (include/lvk_c.h) defines.

A job is one clone b of the window (attitude q_b body to world, position p_b, columns c..c+5 = [d_theta_b d_p_b]) and the extrinsics
(R_b2c, t_c_b, columns 15..20 = [d_theta_e d_t]).  The camera pose is R_wc = R_b R_b2c^T, p_wc = p_b + R_b t_c_b; its error is read
as lvk_map_select_queries reads cov_cam: R_wc,true = R_wc (I + [dtheta]x), p_wc,true = p_wc + dp.  Under the filter's injection
(R_b <- (I + [d_theta_b]x) R_b, p_b <- p_b + d_p_b, R_b2c <- R_b2c R(d_theta_e)^T, t_c_b <- t_c_b + d_t)
    dtheta = R_b2c d_theta_e + R_wc^T d_theta_b,   dp = R_b d_t - [R_b t_c_b]x d_theta_b + d_p_b,   cov_cam = J P_s J^T.

Two routes to J: jacobian_nd(), central differences of the injected pose written from the geometry (no derivative is written down on
that route), and the closed form jacobian().  tests/test_camera_pose_ref.py holds them to each other; the GPU tests compare the kernel
with pose_cov()."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, quat_mul, small_angle_quat, skew

LD = np.longdouble
H_STEP = LD(2.0) ** -21           # central-difference step, as landmark_fix_ref.H_STEP


def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


def make_job(clone_col, q_b, p_b, R_b2c, t_c_b):
    return dict(clone_col=int(clone_col), q_b=np.asarray(q_b, np.float64), p_b=np.asarray(p_b, np.float64), R_b2c=np.asarray(R_b2c, np.float64).reshape(3, 3),
                t_c_b=np.asarray(t_c_b, np.float64))


def columns(job):
    c = job["clone_col"]
    return np.array(list(range(15, 21)) + list(range(c, c + 6)))


def pose(job, d12=None):
    """(R_wc, p_wc) after the injection of d12 = [d_theta_e d_t d_theta_b d_p_b], long double"""
    d = np.zeros(12, LD) if d12 is None else np.asarray(d12, LD)
    q = quat_mul(small_angle_quat(d[6:9]), _ld(job["q_b"])); p = _ld(job["p_b"]) + d[9:12]
    Re = _ld(job["R_b2c"]) @ quat_to_rot(small_angle_quat(d[0:3])).T; t = _ld(job["t_c_b"]) + d[3:6]
    Rb = quat_to_rot(q)
    return Rb @ Re.T, p + Rb @ t


def jacobian(job):
    """6 x 12, the closed form of the header"""
    R_wc, _ = pose(job)
    Rb = quat_to_rot(_ld(job["q_b"])); Re = _ld(job["R_b2c"]); u = Rb @ _ld(job["t_c_b"])
    J = np.zeros((6, 12), LD)
    J[0:3, 0:3] = Re; J[0:3, 6:9] = R_wc.T
    J[3:6, 3:6] = Rb; J[3:6, 6:9] = -skew(u); J[3:6, 9:12] = np.eye(3, dtype=LD)
    return J


def _vee(M):
    return np.array([(M[2, 1] - M[1, 2]) / 2, (M[0, 2] - M[2, 0]) / 2, (M[1, 0] - M[0, 1]) / 2], LD)


def jacobian_nd(job, h=H_STEP):
    """6 x 12: central differences of (vee(R_wc^T R_wc'), p_wc') under the injection - R_wc' = R_wc (I + [dtheta]x) reads dtheta off
    the antisymmetric part of R_wc^T R_wc'"""
    R0, _ = pose(job)
    J = np.zeros((6, 12), LD)
    for k in range(12):
        d = np.zeros(12, LD); d[k] = h
        Rp, pp = pose(job, d); Rm, pm = pose(job, -d)
        J[0:3, k] = _vee(R0.T @ (Rp - Rm)) / (2 * h)
        J[3:6, k] = (pp - pm) / (2 * h)
    return J


def pose_cov(P, job):
    """(R_wc, p_wc, cov_cam = J P_s J^T), long double"""
    R_wc, p_wc = pose(job)
    J = jacobian(job)
    c = columns(job)
    Ps = _ld(P)[np.ix_(c, c)]
    return R_wc, p_wc, J @ Ps @ J.T


# ------------------------------------------------------------------------------------------------ cases
def random_quat(rng):
    q = rng.normal(0, 1, 4)
    return q / np.linalg.norm(q)


def random_rot(rng):
    return np.asarray(quat_to_rot(random_quat(rng)), np.float64)


def random_jobs(seed=11, count=24):
    """`count` random poses and extrinsics; job 0 has t_c_b = 0, job 1 an identity R_b2c, job 2 both"""
    rng = np.random.default_rng(seed)
    jobs = []
    for k in range(count):
        R_e = np.eye(3) if k in (1, 2) else random_rot(rng)
        t_e = np.zeros(3) if k in (0, 2) else rng.uniform(-0.3, 0.3, 3)
        jobs.append(make_job(21 + 6 * int(rng.integers(0, 5)), random_quat(rng), rng.uniform(-5, 5, 3), R_e, t_e))
    return jobs


def random_spd(rng, n):
    """a covariance-like SPD matrix with entries of mixed size (attitude 1e-4, position 1e-2), as a filter's"""
    B = rng.normal(0, 1, (n, n))
    s = 10.0 ** rng.uniform(-3, -1, n)
    P = (B @ B.T / n + np.eye(n)) * np.outer(s, s)
    return (P + P.T) / 2


def stage_cases():
    """the GPU stage's cases: n = 21 + 6 * 3 and 21 + 6 * 5, the clone first, middle and last -> list of (name, P, job)"""
    rng = np.random.default_rng(29)
    out = []
    for n_clones in (3, 5):
        n = 21 + 6 * n_clones
        for rank in (0, n_clones // 2, n_clones - 1):
            P = random_spd(rng, n)
            job = make_job(21 + 6 * rank, random_quat(rng), rng.uniform(-5, 5, 3), random_rot(rng), rng.uniform(-0.3, 0.3, 3))
            out.append((f"n{n}_rank{rank}", P, job))
    return out


def rel_err(a, b):
    """max |a - b| relative to the largest |b|"""
    a = np.asarray(a, LD); b = np.asarray(b, LD)
    return float(np.abs(a - b).max() / np.abs(b).max())
