"""The derivation behind lvk_ekf_camera_pose_cov, on the CPU: the closed-form Jacobian of include/lvk_c.h against central differences of
the injected pose, and larvio_amd.localize's float64 restatement against the long-double one (tests/camera_pose_ref.py)."""
import numpy as np

from larvio_amd import localize
from tests import camera_pose_ref as R

# Central differences with h = 2^-21 in long double.  Truncation: h^2 f''' / 6 = 3.8e-14 f''' (the pose is a product of rotations with
# entries <= 1 and a lever arm <= 0.3 m: f''' is of order 1).  Rounding: a few dozen long-double operations on numbers of size <= 6
# (|p_b| <= 5), 2^-64 each, divided by 2 h = 9.5e-7: a few 1e-13.  Measured on the 24 jobs of random_jobs(): worst |J - J_nd| relative to
# 1 + |t_c_b| = 3.3e-13 (the two difference quotients with h and h / 2 differ by 7.7e-13: rounding dominates, as estimated).  The bound
# is one order of magnitude above the measured value; a wrong sign in any block is an error of order 1.
ND_MEASURED = 3.3e-13
TOL_ND = 10 * ND_MEASURED

# localize.camera_pose_cov_ref against the long-double restatement on the six stage cases: measured worst |a - b| / max |b| = 4.7e-16
# for the covariance (2.1 ulp of the largest entry: sums of twelve products twice over) and 2.1e-16 for the pose.
REF_MEASURED = 4.7e-16
TOL_REF = 8 * np.finfo(np.float64).eps           # "a few ulp of the largest entry": 1.8e-15, four times the measured value


def test_jacobian_signs_by_central_differences():
    """closed form vs central differences, 24 random poses and extrinsics including t_c_b = 0 and an identity R_b2c: measured 3.3e-13"""
    jobs = R.random_jobs()
    assert len(jobs) >= 20
    assert not jobs[0]["t_c_b"].any() and np.array_equal(jobs[1]["R_b2c"], np.eye(3)) and not jobs[2]["t_c_b"].any()
    worst = 0.0
    for job in jobs:
        J, Jn = R.jacobian(job), R.jacobian_nd(job)
        scale = 1 + np.abs(job["t_c_b"]).max()
        worst = max(worst, float(np.abs(J - Jn).max() / scale))
    print(f"closed form vs central differences: worst {worst:.3e} (bound {TOL_ND:.1e})")
    assert worst < TOL_ND


def test_a_wrong_sign_is_seen():
    """the check has teeth: flipping the lever-arm block or the camera-side rotation is an error of order |t_c_b| and 1"""
    job = R.random_jobs()[5]
    J, Jn = R.jacobian(job), R.jacobian_nd(job)
    Jf = J.copy(); Jf[3:6, 6:9] *= -1
    assert np.abs(Jf - Jn).max() > 1e-2
    Jf = J.copy(); Jf[0:3, 6:9] = Jf[0:3, 6:9].T
    assert np.abs(Jf - Jn).max() > 1e-2


def test_rigid_translation_moves_only_dp():
    """d_p_b moves p_wc one to one and leaves R_wc alone; d_t enters through R_b"""
    job = R.random_jobs()[7]
    J = R.jacobian(job)
    assert np.array_equal(J[3:6, 9:12], np.eye(3)) and not J[0:3, 9:12].any() and not J[0:3, 3:6].any() and not J[3:6, 0:3].any()


def test_float64_restatement_against_long_double():
    """localize.camera_pose_cov_ref vs the long-double restatement on the GPU stage's cases: measured 4.7e-16, bound 8 eps"""
    worst = 0.0
    for name, P, job in R.stage_cases():
        Rl, pl, cl = R.pose_cov(P, job)
        Rn, pn, cn = localize.camera_pose_cov_ref(P, job["clone_col"], dict(q=job["q_b"], p=job["p_b"]), (job["R_b2c"], job["t_c_b"]))
        assert np.array_equal(cn, cn.T), name
        worst = max(worst, R.rel_err(cn, cl), R.rel_err(Rn, Rl), R.rel_err(pn, pl))
    print(f"float64 restatement vs long double: worst {worst:.3e} (bound {TOL_REF:.1e})")
    assert worst < TOL_REF


def test_camera_pose_matches_the_restatement():
    """localize.camera_pose is the pose part of camera_pose_cov_ref, bit for bit"""
    name, P, job = R.stage_cases()[0]
    clone = dict(q=job["q_b"], p=job["p_b"]); ext = (job["R_b2c"], job["t_c_b"])
    R_wc, p_wc = localize.camera_pose(clone, ext)
    Rn, pn, _ = localize.camera_pose_cov_ref(P, job["clone_col"], clone, ext)
    assert np.array_equal(R_wc, Rn) and np.array_equal(p_wc, pn)
