"""lvk_ekf_camera_pose_cov (larvio_amd/csrc/be_camera_pose.hip) as a stage: against the long-double restatement
(tests/camera_pose_ref.py), against its float64 restatement bit for bit, with the extrinsics not estimated, with everything outside
the twelve rows and columns poisoned, and every refusal.

The bound.  On the six cases of camera_pose_ref.stage_cases() the float64 numpy restatement (localize.camera_pose_cov_ref) differs from
the long-double one by at most 4.7e-16 of the largest entry (measured; tests/test_camera_pose_ref.py asserts it on the CPU).  The kernel
is held to ten times that value."""
import numpy as np
import pytest

from larvio_amd import localize
from tests import camera_pose_ref as R

pytestmark = pytest.mark.gpu

REF_MEASURED = 4.7e-16            # float64 numpy restatement vs long double, same cases (tests/test_camera_pose_ref.py)
TOL = 10 * REF_MEASURED


def _job(job):
    from larvio_amd import ops
    return ops.camera_pose_job(job["clone_col"], job["q_b"], job["p_b"], job["R_b2c"], job["t_c_b"])


def _ref64(P, job):
    return localize.camera_pose_cov_ref(P, job["clone_col"], dict(q=job["q_b"], p=job["p_b"]), (job["R_b2c"], job["t_c_b"]))


@pytest.fixture(scope="module")
def cases():
    return R.stage_cases()


def test_against_long_double(gpu_ctx, cases):
    """n = 39 and 51, the clone first, middle and last: within 10 x 4.7e-16 of the long-double value, and equal to the float64
    restatement bit for bit (the header fixes every order)"""
    from larvio_amd import ops
    worst = 0.0
    for name, P, job in cases:
        R_wc, p_wc, cov = ops.camera_pose_cov(gpu_ctx, P, _job(job))
        Rl, pl, cl = R.pose_cov(P, job)
        e = max(R.rel_err(cov, cl), R.rel_err(R_wc, Rl), R.rel_err(p_wc, pl))
        print(f"{name}: rel err {e:.3e}")
        worst = max(worst, e)
        assert np.array_equal(cov, cov.T), name
        Rn, pn, cn = _ref64(P, job)
        assert np.array_equal(R_wc, Rn) and np.array_equal(p_wc, pn) and np.array_equal(cov, cn), name
    print(f"worst {worst:.3e} (bound {TOL:.1e})")
    assert worst < TOL


def test_padded_leading_dimension(gpu_ctx, cases):
    """the covariance inside a wider buffer (ldp > n) whose padding is NaN: the same bits"""
    from larvio_amd import ops
    name, P, job = cases[1]
    n = len(P)
    buf = np.full((n + 3, n + 5), np.nan); buf[:n, :n] = P
    a = ops.camera_pose_cov(gpu_ctx, P, _job(job))
    b = ops.camera_pose_cov(gpu_ctx, buf, _job(job), n=n)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_extrinsics_not_estimated(gpu_ctx, cases):
    """a zero extrinsics block: the result is J_b P_bb J_b^T of the clone block alone, symmetric bit for bit"""
    from larvio_amd import ops
    for name, P, job in cases:
        P0 = P.copy(); P0[15:21, :] = 0; P0[:, 15:21] = 0
        _, _, cov = ops.camera_pose_cov(gpu_ctx, P0, _job(job))
        c = job["clone_col"]
        Jb = np.asarray(R.jacobian(job)[:, 6:12], np.float64)                      # the closed form's clone block, rounded to float64
        want = Jb @ P0[c:c + 6, c:c + 6] @ Jb.T
        assert np.array_equal(cov, cov.T), name
        assert np.abs(cov - want).max() <= TOL * np.abs(want).max(), name
        # and bit for bit the sum over the clone's six terms alone, in the header's order
        Rn, pn, cn = _ref64(P0, job)
        assert np.array_equal(cov, cn), name


def test_locality(gpu_ctx, cases):
    """NaN everywhere outside the twelve rows and columns: the result keeps its bits"""
    from larvio_amd import ops
    for name, P, job in cases:
        cols = R.columns(job)
        Q = np.full_like(P, np.nan)
        Q[np.ix_(cols, cols)] = P[np.ix_(cols, cols)]
        a = ops.camera_pose_cov(gpu_ctx, P, _job(job))
        b = ops.camera_pose_cov(gpu_ctx, Q, _job(job))
        assert all(np.isfinite(x).all() for x in b), name
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name


def test_refusals(gpu_ctx, cases):
    """every refusal is LVK_ERR_ARG, leaves the outputs untouched, and the context goes on"""
    import ctypes as C
    from larvio_amd import ops
    from larvio_amd._lib import lib, _p
    name, P, job = cases[0]
    n = len(P)
    good = _job(job)

    def refused(j, P=P, n=None):
        st, (R_wc, p_wc, cov) = ops.camera_pose_cov(gpu_ctx, P, j, n=n, check=False)
        assert st == 1, st
        assert np.isnan(R_wc).all() and np.isnan(p_wc).all() and np.isnan(cov).all()

    for col in (20, 0, -1, n - 5, n):
        j = good.copy(); j["clone_col"] = col; refused(j)
    for field, k in (("q_b", 0), ("p_b", 1), ("R_b2c", 4), ("t_c_b", 2)):
        for bad in (np.nan, np.inf):
            j = good.copy(); j[field][0, k] = bad; refused(j)
    j = good.copy(); j["q_b"] *= 1 + 3e-6; refused(j)
    j = good.copy(); j["q_b"] *= 1 + 5e-7
    assert ops.camera_pose_cov(gpu_ctx, P, j, check=False)[0] == 0             # inside 1e-6: accepted
    refused(good, n=n + 1)                                                     # ldp < n
    L = lib()
    dP = gpu_ctx.to_device(P); out = np.zeros(48)
    args = [gpu_ctx.h, _p(dP), n, n, _p(good), _p(out[:9]), _p(out[9:12]), _p(out[12:])]
    for k in (1, 4, 5, 6, 7):
        a = list(args); a[k] = None
        assert L.lvk_ekf_camera_pose_cov(*a) == 1
    assert L.lvk_ekf_camera_pose_cov(None, *args[1:]) == 1
    assert b"lvk_ekf_camera_pose_cov" in L.lvk_last_error(gpu_ctx.h)
    # the context goes on
    a = ops.camera_pose_cov(gpu_ctx, P, good)
    assert np.array_equal(a[2], _ref64(P, job)[2])
