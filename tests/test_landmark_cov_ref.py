"""CPU pins of tests/landmark_cov_ref.py, the long-double restatement the GPU tests of lvk_ekf_landmark_cov compare against: its
quaternion helpers against be_host_math.h compiled on the host, its composition (injection + position formula, differentiated
numerically) against closed forms that hold whatever the sign or side conventions are, and the error of its own differentiation,
which sets the tolerance the GPU tests use."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import landmark_cov_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = R.LD


def _jobs(seed, n):
    rng = np.random.default_rng(seed)
    depths = np.concatenate([[0.5, 5.0], rng.uniform(0.5, 5.0, n - 2)])
    return [R.random_job(rng, 22, 34, depth=d) for d in depths]


def test_helpers_equal_the_products_host_math(tmp_path):
    """quat_to_rot, rot_to_quat (all four branches), quat_mul, small_angle_quat (both branches) and skew in float64 against
    tests/host/host_math_dump.hip, which prints what larvio_amd/csrc/be_host_math.h computes for 200 seeded inputs"""
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "host_math_dump")
    flags = ["-O2", "-std=c++17", "-ffp-contract=off", "-w", "-x", "c++"] if cxx.endswith("g++") else ["-O2", "-std=c++17", "-ffp-contract=off", "-w", "-x", "hip", "--offload-arch=gfx950"]
    subprocess.check_call([cxx] + flags + [os.path.join(ROOT, "tests", "host", "host_math_dump.hip"), "-o", exe])
    rows = [json.loads(l) for l in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert len(rows) == 200
    neg_trace = big_angle = 0
    for r in rows:
        q, p, w = np.array(r["q"]), np.array(r["p"]), np.array(r["w"])
        Rm = R.quat_to_rot(q)
        assert np.abs(Rm - np.reshape(r["R"], (3, 3))).max() <= 4e-16
        neg_trace += np.trace(Rm) <= 0
        assert np.abs(R.rot_to_quat(np.reshape(r["R"], (3, 3))) - np.array(r["q2"])).max() <= 4e-16        # same branch, same sign
        assert np.abs(R.quat_mul(q, p) - np.array(r["qp"])).max() <= 1e-15
        assert np.abs(R.small_angle_quat(w) - np.array(r["dq"])).max() <= 4e-16
        big_angle += (w @ w) / 4 > 1
        assert np.array_equal(R.skew(w), np.reshape(r["S"], (3, 3)))
    assert neg_trace >= 20 and big_angle >= 5


def _block_only(lo, hi, s2):
    Ps = np.zeros((R.N_ERR, R.N_ERR), LD)
    for k in range(lo, hi):
        Ps[k, k] = s2
    return Ps


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_closed_forms_of_isotropic_blocks(seed):
    """one isotropic block s^2 I of P_s alone: anchor position and extrinsic translation give s^2 I; anchor attitude s^2 [r]x [r]x^T with
    r = p_w - p_clone; extrinsic rotation s^2 [r_c]x [r_c]x^T with r_c = p_w - p_cam; rho alone sigma^2 d d^T, d = (p_w - p_cam) / rho.
    None of these depends on which side a rotation error multiplies from or on its sign.
    Tolerance: a central difference leaves an ABSOLUTE error in every entry of J (rounding of p_w over 2h, truncation), TOL_ND being
    its measured size relative to the entries that carry weight.  With one block alone an entry of B = |J| |P_s| |J|^T can be
    arbitrarily small (r nearly along an axis makes two entries of [r]x tiny), which that absolute error does not follow; so the
    scale is B plus s^2 k m^2, k the block's width and m its largest |J| entry - the size B has where the block is not degenerate."""
    s2 = LD(1e-4)
    for job in _jobs(seed, 6):
        p_clone, p_cam, _, rho = R.poses(job)
        p_w = R.position(job)
        J = R.jacobian_nd(job)
        r, r_c = p_w - p_clone, p_w - p_cam
        cases = [(9, 12, s2 * np.eye(3, dtype=LD)), (6, 9, s2 * R.skew(r) @ R.skew(r).T), (3, 6, s2 * np.eye(3, dtype=LD)),
                 (0, 3, s2 * R.skew(r_c) @ R.skew(r_c).T), (12, 13, s2 * np.outer(r_c / rho, r_c / rho))]
        for lo, hi, want in cases:
            Ps = _block_only(lo, hi, s2)
            got = R.sigma_from(J, Ps); B = R.bound(J, Ps)
            scale = B + s2 * (hi - lo) * np.abs(J[:, lo:hi]).max() ** 2
            assert np.all(np.abs(got - want) <= R.TOL_ND * scale), (lo, hi, float(np.max(np.abs(got - want) / scale)))


def test_differentiation_error_sets_tol_nd():
    """central differences at H_STEP and at H_STEP / 2 on landmarks 0.5 - 5 m deep (both ends included), random SPD P_s:
    10 x the largest difference relative to B is the tolerance the GPU tests use"""
    worst = 0.0
    rng = np.random.default_rng(11)
    for job in _jobs(3, 24):
        P = R.random_spd(rng, 35)
        S1, B, _ = R.sigma(job, P, R.H_STEP)
        S2, _, _ = R.sigma(job, P, R.H_STEP / 2)
        worst = max(worst, float(np.max(np.abs(S1 - S2) / B)))
    print("central differences, h vs h/2: worst |dSigma| / B = %.3g; TOL_ND = %.3g" % (worst, R.TOL_ND))
    assert 10 * worst <= R.TOL_ND <= 1e-9
