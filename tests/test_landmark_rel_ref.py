"""The restatement the GPU tests of lvk_ekf_landmark_rel_cov compare against (tests/landmark_rel_ref.py), held to itself on the CPU: its
closed form against central differences of p_c written from the geometry, the closed-form special cases (zero, pure gauge, target equal
to anchor), the size of the derived bound and its power to tell three seeded mistakes from the truth on every problem the GPU tests use,
and the consistency of Sigma on the oracle's filter against the simulation's true landmarks in the true camera frame.

Filter-level consistency, measured here with the oracle's filter (feature_sim.simulate(4, t1=6.0, sw_size=10, fresh_ids=True), every
in-state feature after every message, target the IMU state): d2 = e^T Sigma^-1 e over three degrees of freedom has the quantiles
printed by test_camera_frame_covariance_is_consistent_on_the_oracles_filter; its median stays below 16.27 (see PARITY.md)."""
import numpy as np
import pytest

from tests import landmark_rel_ref as R

LD = R.LD


def _jobs():
    return [(L, k, j) for L in R.stage_launches() for k, j in enumerate(L["jobs"])]


@pytest.fixture(scope="module")
def tracked():
    """(launch, job index, job, p_c, err_p, Sigma, err, Bnd) of every job of the GPU stage tests, computed once"""
    return [(L, k, j) + R.tracked(j, L["P"]) for L, k, j in _jobs()]


def _scale(j):
    _, _, _, _, f_A, _, _, g, _, _ = R.geometry(j)
    return 1 + float(np.linalg.norm(f_A)) + float(np.linalg.norm(g)) + float(np.linalg.norm(j["t_c_b"]))


def test_the_launches_cover_the_shapes_and_job_counts():
    Ls = R.stage_launches()
    assert {L["n"] for L in Ls} == {29, 58, 60, 433} and {L["ldp"] - L["n"] for L in Ls} == {0, R.PAD}
    assert {len(L["jobs"]) for L in Ls if L["n"] == 433} == {1, 65, 300}
    jobs = [(L, j) for L in Ls for j in L["jobs"]]
    assert any(L["n"] == 29 and j["a"] is j["b"] for L, j in jobs) and any(L["n"] == 29 and (j["b"][0], j["b"][1]) == (0, 6) for L, j in jobs)
    assert any(L["n"] == 58 and L["ldp"] > 58 and j["feat_col"] == 57 for L, j in jobs)
    depth = np.array([1 / j["rho"] for _, j in jobs])
    assert depth.min() < 0.5 and depth.max() > 20 and depth.min() >= 0.3 and depth.max() <= 30


def test_closed_form_J_equals_the_central_difference_J():
    worst = 0.0; n = 0
    for L in R.stage_launches():
        for j in L["jobs"][:10]:
            J_nd = R.merged(j, R.jacobian_nd(j), nd=True); J_cf = R.merged(j, R.jacobian_closed(j), nd=False)
            s = _scale(j)
            d = np.abs(J_nd - J_cf) / s
            d[:, 18] *= j["rho"]                          # d p_c / d rho is relative to s / rho
            worst = max(worst, float(d.max())); n += 1
    print("%d jobs: largest |J_nd - J_closed| / s = %.2e (TOL_ND %.0e)" % (n, worst, R.TOL_ND))
    assert n >= 25 and worst < R.TOL_ND


def test_the_two_routes_agree_on_every_gpu_problem(tracked):
    """Sigma by central differences against Sigma by the closed form.  The tolerance follows from the step size through TOL_ND: the two
    J's differ entrywise by at most E = TOL_ND s w^T (w = 1, for rho's column 1 / rho: landmark_rel_ref.TOL_ND), so the two Sigma differ
    by at most E |P_s| |J|^T + |J| |P_s| E^T + E |P_s| E^T, entrywise.  p_c of the geometry route equals the tracked route's value
    to long-double rounding (64 u_ld s: some forty operations on numbers of size s)."""
    worst = 0.0; n = 0
    for L, k, j, pc, err_p, S, err, Bnd in tracked:
        s = _scale(j)
        E = np.full((3, R.N_ERR), LD(R.TOL_ND * s)); E[:, 18] /= LD(j["rho"])
        Ps = np.abs(R.gather(L["P"], j)); J = np.abs(R.jacobian_closed(j))
        tol = E @ Ps @ J.T + J @ Ps @ E.T + E @ Ps @ E.T
        worst = max(worst, float(np.max(np.abs(R.sigma_nd(j, L["P"]) - S) / tol))); n += 1
        assert np.max(np.abs(R.point_in_camera(j) - pc)) <= 64 * float(R.U_LD) * s
    print("%d jobs: largest |Sigma_nd - Sigma_closed| / (the tolerance TOL_ND gives) %.3g" % (n, worst))
    assert n >= 30 and worst <= 1.0


def test_zero_covariance_gives_zero(tracked):
    for L, k, j, *_ in tracked[:10]:
        Z = np.zeros_like(L["P"])
        _, _, S0, err0, Bnd0 = R.tracked(j, Z)
        assert np.all(S0 == 0) and np.all(err0 == 0) and np.all(Bnd0 == 0)
        assert np.all(R.sigma_nd(j, Z) == 0)


def test_pure_gauge_covariance_cancels_inside_the_bound():
    """P = G (1e2 I) G^T, a rotation of the world about z and a translation over every pose slot: every camera-frame covariance is zero
    to the rounding the bound allows"""
    worst = 0.0
    for L in R.stage_launches():
        P = R.with_gauge(np.zeros_like(L["P"]), L["slots"])
        for j in L["jobs"][:12]:
            _, _, S, err, Bnd = R.tracked(j, P)
            assert Bnd.max() >= R.GAUGE_VAR                # ... of something large
            assert np.all(np.abs(S) <= err), L["name"]
            worst = max(worst, float(np.max(np.abs(S) / err)))
    print("pure gauge: largest |Sigma| / bound %.3g" % worst)


def test_target_equal_to_anchor_gives_the_depth_term_alone(tracked):
    n = 0
    for L, k, j, pc, err_p, S, err, Bnd in tracked:
        if j["a"] is not j["b"]:
            continue
        rho = LD(j["rho"]); u, v = R._ld(j["obs"])
        f_A = np.array([u / rho, v / rho, 1 / rho], LD)
        want = LD(L["P"][j["feat_col"], j["feat_col"]]) * np.outer(f_A, f_A) / (rho * rho)
        assert np.all(np.abs(S - want) <= err), (L["name"], k)
        assert np.all(np.abs(pc - f_A) <= err_p)
        n += 1
    assert n >= 5


def test_the_bound_is_small_against_the_scale_of_every_gpu_problem(tracked):
    worst = 0.0
    for L, k, j, pc, err_p, S, err, Bnd in tracked:
        assert np.all(np.isfinite(S.astype(np.float64))) and np.all(err > 0) and np.all(err_p > 0)
        r = float(np.max(err / Bnd)); worst = max(worst, r)
        assert r <= 1e-10, (L["name"], k, r)
        assert np.all(err_p <= 1e-12 * _scale(j))
    print("%d jobs: largest bound / (|J| |P_s| |J|^T) %.3g" % (len(tracked), worst))


@pytest.mark.parametrize("mutation", ("sign", "swap", "plus3"))
def test_seeded_mutations_exceed_the_bound_on_every_problem_they_apply_to(tracked, mutation):
    """the sign of the M [g]x block; the anchor's and the target's blocks of J exchanged; the target's position columns taken as theta + 3
    when the target is the IMU state"""
    n = 0; least = np.inf
    for L, k, j, pc, err_p, S, err, Bnd in tracked:
        a, b = j["a"], j["b"]
        if mutation == "swap" and a is b:
            continue                                      # (the same columns twice: exchanging their blocks changes nothing)
        if mutation == "plus3" and b[1] == b[0] + 3:
            continue
        r = float(np.max(np.abs(R.sigma(j, L["P"], mutate=mutation) - S) / err))
        least = min(least, r); n += 1
        assert r > 1.0, (L["name"], k, mutation, r)
    print("%s: %d problems, smallest |mutated - Sigma| / bound %.3g" % (mutation, n, least))
    assert n >= (50 if mutation == "plus3" else 200)


def test_camera_frame_covariance_is_consistent_on_the_oracles_filter():
    """Sigma of every in-state feature of the oracle's filter in the camera frame of the IMU state, after every message, against the
    simulation's true landmark in the true camera frame at the state's time: d2 = e^T Sigma^-1 e, three degrees of freedom; and what
    the feature is for - the trace of the world-frame Sigma (tests/landmark_cov_ref.py) against the camera-frame one at the last message"""
    from oracle import lvo_be
    from tests import feature_sim as F
    from tests import landmark_cov_ref as W
    sim = F.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)
    ekf = lvo_be.Ekf(sim["cfg"])
    d2 = []; last = {}

    def on_update(ts):
        P = ekf.cov(); cl = ekf.clones(); st = ekf.state(); ids, idp, pos = ekf.features()
        jobs, rows = R.filter_jobs(st, cl, ids, idp, pos)
        R_wc, p_wc = sim["traj"].cam_pose(st["t"])
        tr_w, tr_c = [], []
        for j, i in zip(jobs, rows):
            S = R.sigma(j, P).astype(np.float64)
            assert np.max(np.abs(S - S.T)) <= 1e-12 * np.abs(S).max()
            S = (S + S.T) / 2
            assert np.linalg.eigvalsh(S).min() > 0
            e = np.asarray(R.point_in_camera(j), np.float64) - R_wc.T @ (sim["landmarks"][ids[i]] - p_wc)
            d2.append(float(e @ np.linalg.solve(S, e)))
            wj = dict(anchor_col=j["a"][0], feat_col=j["feat_col"], q_anchor=j["a"][2], R_b2c=j["R_b2c"].ravel(), t_c_b=j["t_c_b"], obs_anchor=j["obs"], inv_depth=j["rho"])
            tr_w.append(float(np.trace(W.sigma(wj, P)[0]))); tr_c.append(float(np.trace(S)))
        last["ratio"] = np.array(tr_w) / np.array(tr_c); last["n"] = len(ids); last["used"] = len(rows); last["sd"] = np.sqrt(np.array(tr_c))
    n = F.drive(ekf, sim, on_update)
    d2 = np.array(d2)
    q = np.quantile(d2, [0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
    print("%d updates, %d feature-messages; d2 = e^T Sigma^-1 e: 10/25/50/75/90/99 %% = %s, share below %.2f: %.3f" % (n, len(d2), np.array2string(q, precision=3), R.CHI2_3_999,
                                                                                                                 np.mean(d2 < R.CHI2_3_999)))
    r = last["ratio"]
    print("last message: %d of %d features; trace Sigma_world / trace Sigma_cam: min %.3g median %.3g max %.3g; sqrt(trace Sigma_cam) median %.3g m"
          % (last["used"], last["n"], r.min(), np.median(r), r.max(), np.median(last["sd"])))
    assert n >= 40 and len(d2) > 200
    assert np.median(d2) < R.CHI2_3_999
