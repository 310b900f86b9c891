"""The restatement the GPU tests of lvk_ekf_update_landmarks and lvk_ekf_add_landmark_obs compare against (tests/landmark_fix_ref.py),
held to itself on the CPU: the closed-form H and d h / d p_w against central differences of h under the filter's injection, a batch
with nothing gated against the literal K = P H^T (H P H^T + R)^-1 of the uncompressed rows, the extrinsics columns under a zero
extrinsics block, the residual under a rigid shift of the world, the distance of every gamma_k from its gate and of every depth from
min_depth, the size of the derived bound and its power to tell three seeded mistakes from the truth on every problem of the GPU stage
tests they apply to."""
import numpy as np
import pytest

from tests import landmark_fix_ref as R
from tests.landmark_cov_ref import quat_to_rot, quat_mul

LD = R.LD


@pytest.fixture(scope="module")
def tracked():
    return R.stage_tracked()


def test_the_problems_cover_what_the_issue_lists(tracked):
    ps = [pr for pr, _ in tracked]
    assert {len(p["obs"]) for p in ps} >= {1, 5, 6, 7, 63, 64, 65, 256, 257, 1024}
    assert {p["n"] for p in ps} == {28, 216, 433} and {p["ldp"] - p["n"] for p in ps} == {0, R.PAD}
    assert any(p["n"] == 28 and p["job"]["clone_col"] == 22 for p in ps)
    for n in (216, 433):
        cc = {p["job"]["clone_col"] for p in ps if p["n"] == n}
        assert 22 in cc and max(cc) + 6 >= n - 6 and any(22 < c < n - 12 for c in cc)       # first, last (or next to the feature columns), middle
    assert any(t["n_used"] and t["n_gated"] and t["n_behind"] for _, t in tracked)
    assert {t["m"] for _, t in tracked} >= {2, 10, 12, 6}
    assert any(p["zero_cov"] for p in ps) and any(np.all(p["P"][15:21] == 0) for p in ps)


def test_closed_form_H_equals_the_central_difference_H(tracked):
    worst = 0.0; n = 0
    for pr, _ in tracked:
        for ob in pr["obs"][:6]:
            row = R.obs_rows(pr["job"], ob)
            if row["status"] == R.BEHIND:
                continue
            g = np.linalg.norm(ob["p_w"] - pr["job"]["p_b"]); z = float(row["pc"].v[2])
            scale = (1 + g) / z
            worst = max(worst, float(np.max(np.abs(R.jacobian_nd(pr["job"], ob["p_w"]) - row["H"].v))) / scale,
                        float(np.max(np.abs(R.point_jacobian_nd(pr["job"], ob["p_w"]) - row["JM"].v))) / scale)
            n += 1
    print("%d observations: largest |H_nd - H_closed| z / (1 + |g|) = %.2e (TOL_ND %.0e)" % (n, worst, R.TOL_ND))
    assert n >= 40 and worst < R.TOL_ND


def test_residual_reads_back_a_small_injected_error(tracked):
    pr, _ = tracked[5]
    d = 1e-6 * np.arange(1, 13).astype(LD)
    for ob in pr["obs"][:5]:
        row = R.obs_rows(pr["job"], ob)
        ob2 = ob.copy(); ob2["uv"] = R.project(R.cam_point(pr["job"], ob["p_w"], d)).astype(np.float64)
        r = R.obs_rows(pr["job"], ob2)["r"].v
        assert np.max(np.abs(r - row["H"].v @ d)) < 1e-9                      # second order: (1.2e-5)^2 times a few
        ob2["uv"] = R.project(R.cam_point(pr["job"], ob["p_w"])).astype(np.float64)
        assert np.max(np.abs(R.obs_rows(pr["job"], ob2)["r"].v)) < 1e-15


def test_a_batch_with_nothing_gated_equals_the_literal_gain_of_the_uncompressed_rows(tracked):
    """another order of operations in the same long double (no whitening, no compression, S of 2 n_used rows): the two differ by this
    file's own rounding only, which the bound derived for float64 covers with room"""
    worst = 0.0; n = 0
    for pr, t in tracked:
        if pr["mixed"] or len(pr["obs"]) > 300:
            continue
        p = R.batch_plain(pr["P"], pr["job"], pr["obs"])
        assert np.array_equal(p["status"], t["status"]) and np.all(t["status"] == R.USED)
        w = max(R.worst_ratio(p["dx"] - t["dx"], t["e_dx"]), R.worst_ratio(p["P"] - t["P"], t["e_P"]), R.worst_ratio(p["gamma"] - t["gamma"], t["e_gamma"]))
        worst = max(worst, w); n += 1
        assert w <= 1.0, (pr["name"], w)
        # ... and, loosely, in float64 terms: the same numbers to 1e-6 of their scale
        assert np.max(np.abs(p["dx"] - t["dx"])) <= 1e-6 * np.max(np.abs(t["dx"])) and np.max(np.abs(p["P"] - t["P"])) <= 1e-9 * np.max(np.abs(t["P"])), pr["name"]
    print("literal gain: %d problems, largest |difference| / bound %.3g" % (n, worst))
    assert n >= 8


def test_with_a_zero_extrinsics_block_the_extrinsics_columns_change_nothing(tracked):
    pr, t = next((pr, t) for pr, t in tracked if np.all(pr["P"][15:21] == 0))
    assert t["batch_status"] == 0 and np.all(t["dx"][15:21] == 0) and np.all(t["P"][15:21] == 0) and np.all(t["P"][:, 15:21] == 0)
    a = R.batch_plain(pr["P"], pr["job"], pr["obs"]); b = R.batch_plain(pr["P"], pr["job"], pr["obs"], drop_extrinsics=True)
    assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["P"], b["P"]) and np.array_equal(a["gamma"], b["gamma"])


def test_a_rigid_shift_of_the_world_with_the_points_leaves_the_residual(tracked):
    """in long double throughout (nothing is rounded to float64 after the shift): 1 km and 0.7 rad of yaw"""
    pr, _ = tracked[4]
    job = pr["job"]
    qz = np.array([0, 0, np.sin(LD(0.35)), np.cos(LD(0.35))], LD); Rz = quat_to_rot(qz); t = np.array([1000, -700, 30], LD)

    def resid(q_b, p_b, p_w, uv):
        pc = job["R_b2c"].astype(LD) @ (quat_to_rot(q_b).T @ (p_w - p_b) - job["t_c_b"].astype(LD))
        return uv.astype(LD) - R.project(pc)
    q0 = job["q_b"].astype(LD); p0 = job["p_b"].astype(LD)
    for ob in pr["obs"][:10]:
        pw = ob["p_w"].astype(LD)
        d = resid(q0, p0, pw, ob["uv"]) - resid(quat_mul(qz, q0), Rz @ p0 + t, Rz @ pw + t, ob["uv"])
        assert np.max(np.abs(d)) < 1e-12                  # 2^-64 * 1e3 m * a few operations / depth
    # ... and through the kernel's order of operations - g = p_w - p_b first - with the shifted inputs rounded to float64: the shift costs
    # the rounding of the inputs (half an ulp of 4096 m, 4.5e-13, on each of p_w and p_b, divided by a depth >= 1.5 m) and nothing more
    sh = np.array([4096.0, -2048.0, 512.0])
    j2 = dict(job); j2["p_b"] = job["p_b"] + sh
    for ob in pr["obs"][:10]:
        o2 = ob.copy(); o2["p_w"] = ob["p_w"] + sh
        assert np.max(np.abs(R.obs_rows(j2, o2)["r"].v - R.obs_rows(job, ob)["r"].v)) < 4 * 4.5e-13


def test_no_gamma_is_near_its_gate_and_no_depth_near_min_depth(tracked):
    seen = set()
    for pr, t in tracked:
        gate = pr["job"]["gate"]
        assert t["depth_margin"] > 1e-6, pr["name"]
        if gate > 0:
            live = t["status"] != R.BEHIND
            assert np.all(np.abs(t["gamma"][live].astype(np.float64) - gate) > 1e-6 * gate), pr["name"]
            assert np.all(t["e_gamma"][live] < 1e-6 * gate), pr["name"]
        seen |= {(gate > 0, int(s)) for s in t["status"]}
        assert t["batch_status"] == 0
    assert seen >= {(True, 0), (True, 1), (True, 2), (False, 0)}


def test_the_bounds_are_small_against_the_scale_of_every_gpu_problem(tracked):
    """u cond(S) k: 1.1e-16, S from 1 up to |H_w|^2 |P| = (5 / 2e-3)^2 * 1e2 * 2 n_used / 12 = 1e11 at 1024 observations, a few dozen
    operations: 1e-3 at the outside for P, and for dx and the batch's gamma 1e-2 and 1e-3 of their own size.  The one problem whose
    extrinsics block is zero is the exception: its bound is 0.2 of dx and 0.12 of gamma (printed) - still short of either, so that a dx
    of zero or a residual column summed wrongly lies outside the bound on every problem, compressed or not.  What this asserts is the
    power of the comparison the GPU tests make, not anything the kernels compute."""
    worst = 0.0
    for pr, t in tracked:
        assert np.all(np.isfinite(t["P"].astype(np.float64))) and np.all(t["e_dx"] >= 0) and np.all(t["e_P"] >= 0)
        rP = float(np.max(t["e_P"]) / np.max(np.abs(t["P"]))); rdx = float(np.max(t["e_dx"]) / np.max(np.abs(t["dx"])))
        rg = float(t["e_gamma_b"] / t["gamma_b"])
        print("%-18s m %2d bound / scale: P %.2e dx %.2e batch gamma %.2e (gamma %.4g)" % (pr["name"], t["m"], rP, rdx, rg, float(t["gamma_b"])))
        worst = max(worst, rP)
        no_ext = np.all(pr["P"][15:21] == 0)
        assert rP <= (1e-2 if no_ext else 1e-3), (pr["name"], rP)
        assert rdx <= (0.5 if no_ext else 1e-2) and rg <= (0.5 if no_ext else 1e-3), (pr["name"], rdx, rg)
        assert R.worst_ratio(t["dx"], np.where(t["e_dx"] > 0, t["e_dx"], np.inf)) > 1.0, pr["name"]           # dx = 0 would be told
    print("largest bound / scale of P %.3g" % worst)


def test_every_compressed_problem_has_rank_6_decided_far_from_the_threshold(tracked):
    """the decision is discrete: what a dependent column keeps (rounding) and what an independent one keeps (geometry) both stand off
    RANK_TOL2 by 2^20 and more in the squared norm, so float64 and long double decide alike"""
    n = 0
    for pr, t in tracked:
        if t["n_used"] <= 6:
            assert t["m"] == 2 * t["n_used"]
            continue
        print("%-18s rank %d, decisions off the threshold by a factor %.3g" % (pr["name"], t["m"], t["rank_margin"]))
        assert t["m"] == 6 and t["rank_margin"] > 2.0 ** 20, pr["name"]
        n += 1
    assert n >= 8


def test_a_wrong_residual_column_exceeds_the_bound_on_the_large_batches(tracked):
    """one observation's residual left out of the stacked system (what a sum across wavefronts that loses a term would do), at 65, 257
    and 1024 observations: dx leaves the bound on all three, the batch's gamma on the two whose extrinsics are estimated (with a zero
    extrinsics block the bound on gamma is 0.12 of gamma, and one residual of 65 moves it by as much: printed)"""
    for k in (6, 9, 10):
        pr, t = tracked[k]
        assert len(pr["obs"]) in (65, 257, 1024)
        obs = pr["obs"].copy()
        row = R.obs_rows(pr["job"], obs[-1])
        obs["uv"][-1] = (obs["uv"][-1].astype(LD) - row["r"].v).astype(np.float64)               # its residual becomes zero
        bad = R.batch_tracked(pr["P"], pr["job"], obs)
        assert np.array_equal(bad["status"], t["status"])
        rd = R.worst_ratio(bad["dx"] - t["dx"], np.where(t["e_dx"] > 0, t["e_dx"], np.inf)); rg = float(abs(bad["gamma_b"] - t["gamma_b"]) / t["e_gamma_b"])
        print("%-18s one residual of %d lost: |dx - truth| / bound %.3g, batch gamma %.3g" % (pr["name"], len(obs), rd, rg))
        assert rd > 1.0 and (rg > 1.0 or np.all(pr["P"][15:21] == 0)), pr["name"]


@pytest.mark.parametrize("mutation", ("sign_g", "no_cov", "swap_clone"))
def test_seeded_mistakes_exceed_the_bound_on_every_problem_they_apply_to(tracked, mutation):
    """the sign of [g]x; Sigma_w left out of R_k; the clone's d_theta and d_p blocks swapped - each on the true batch's used observations"""
    n = 0; least = np.inf
    for pr, t in tracked:
        if mutation == "no_cov" and pr["zero_cov"]:
            continue
        if len(pr["obs"]) <= 300:
            bad = R.batch_plain(pr["P"], pr["job"], pr["obs"], mutate=mutation, status=t["status"])
        else:                                         # (ungated: the same observations; the literal form would factor 2048 x 2048 in long double)
            assert not pr["job"]["gate"] > 0
            bad = R.batch_tracked(pr["P"], pr["job"], pr["obs"], mutate=mutation)
        ratio = max(R.worst_ratio(bad["dx"] - t["dx"], np.where(t["e_dx"] > 0, t["e_dx"], np.inf)), R.worst_ratio(bad["P"] - t["P"], np.where(t["e_P"] > 0, t["e_P"], np.inf)))
        least = min(least, ratio); n += 1
        assert ratio > 1.0, (pr["name"], mutation, ratio)
    print("%s: %d problems, smallest |mutated - truth| / bound %.3g" % (mutation, n, least))
    assert n >= 12
