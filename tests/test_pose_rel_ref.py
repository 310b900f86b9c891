"""The restatement the GPU tests of lvk_ekf_pose_rel_cov compare against (tests/pose_rel_ref.py), held to itself on the CPU: its closed
form against central differences of the relative pose written from the geometry, the closed-form special cases (zero, independent
isotropic blocks, pure gauge, a == b), the size of the derived bound and its power to tell three seeded mistakes from the truth on every
problem the GPU tests use, and the consistency of Sigma_rel on the oracle's filter against the simulation's true trajectory.

Filter-level consistency, measured here with the oracle's filter (feature_sim.simulate(4, t1=6.0, sw_size=10, fresh_ids=True), consecutive
clones after every message): d2 = e^T Sigma_rel^-1 e over six degrees of freedom has the quantiles printed by
test_relative_covariance_is_consistent_on_the_oracles_filter; its median stays below 22.46 (see PARITY.md)."""
import numpy as np
import pytest

from tests import pose_rel_ref as R

LD = R.LD


def _rel_jobs():
    return [(L, k, j) for L in R.stage_launches() for k, j in enumerate(L["jobs"]) if j["a"] is not None]


@pytest.fixture(scope="module")
def tracked():
    """(launch, job index, job, Sigma, err, Bnd) of every relative job of the GPU stage tests, computed once"""
    return [(L, k, j) + R.sigma_tracked(j, L["P"]) for L, k, j in _rel_jobs()]


def test_closed_form_J_equals_the_central_difference_J():
    worst = 0.0; n = 0
    for L in R.stage_launches():
        for j in L["jobs"][:8]:
            if j["a"] is None:
                continue
            a, b = j["a"], j["b"]
            J_nd = R.jacobian_nd(a, b); J_cf = R.jacobian_closed(a, b)
            if a is b:                                    # the slot moves as one: what is compared is J [x; x]
                J_cf = J_cf[:, :6] + J_cf[:, 6:]; J_nd = J_nd[:, :6]
            d = float(np.linalg.norm(np.asarray(b[3]) - np.asarray(a[3])))
            worst = max(worst, float(np.max(np.abs(J_nd - J_cf))) / (1 + d)); n += 1
    print("%d jobs: largest |J_nd - J_closed| / (1 + |d|) = %.2e (TOL_ND %.0e)" % (n, worst, R.TOL_ND))
    assert n >= 15 and worst < R.TOL_ND


def test_zero_covariance_gives_zero(tracked):
    for L, k, j, S, err, Bnd in tracked[:10]:
        Z = np.zeros_like(L["P"])
        S0, err0, Bnd0 = R.sigma_tracked(j, Z)
        assert np.all(S0 == 0) and np.all(err0 == 0) and np.all(Bnd0 == 0)
        assert np.all(R.sigma_nd(j, Z) == 0)


def test_independent_isotropic_blocks_have_the_closed_form():
    rng = np.random.default_rng(5)
    st2, sp2 = 3e-4, 2e-3
    for _ in range(6):
        a = R.random_slot(rng, 0, 6); b = R.random_slot(rng, 22, 25)
        P = np.zeros((28, 28))
        for s in (a, b):
            P[s[0]:s[0] + 3, s[0]:s[0] + 3] = st2 * np.eye(3); P[s[1]:s[1] + 3, s[1]:s[1] + 3] = sp2 * np.eye(3)
        job = R.rel(a, b)
        S, err, Bnd = R.sigma_tracked(job, P)
        Ra = R.quat_to_rot(R._ld(a[2])); d = R._ld(b[3]) - R._ld(a[3])
        I = np.eye(3, dtype=LD)
        want_pp = 2 * LD(st2) * I
        want_rr = 2 * LD(sp2) * I + LD(st2) * Ra.T @ ((d @ d) * I - np.outer(d, d)) @ Ra
        tol = 1e-17 * (1 + float(d @ d))                  # long-double rounding of a dozen operations on numbers of size st2 |d|^2
        assert np.max(np.abs(S[:3, :3] - want_pp)) < tol and np.max(np.abs(S[3:, 3:] - want_rr)) < tol
        Snd = R.sigma_nd(job, P)
        assert np.max(np.abs(Snd - S) / Bnd.max()) < 10 * R.TOL_ND * (1 + float(np.sqrt(d @ d)))


def test_pure_gauge_covariance_cancels_inside_the_bound(tracked):
    """P = G Sigma_g G^T, a rigid motion of the world: every relative covariance is zero to the rounding the bound allows"""
    worst = 0.0
    for L in R.stage_launches():
        P = R.with_gauge(np.zeros_like(L["P"]), L["slots"])
        for j in L["jobs"][:12]:
            if j["a"] is None:
                continue
            S, err, Bnd = R.sigma_tracked(j, P)
            assert Bnd.max() >= R.GAUGE_VAR                # ... of something large
            assert np.all(np.abs(S) <= err), L["name"]
            worst = max(worst, float(np.max(np.abs(S) / err)))
    print("pure gauge: largest |Sigma_rel| / bound %.3g" % worst)


def test_a_equal_to_b_gives_zero_inside_the_bound(tracked):
    n = 0
    for L, k, j, S, err, Bnd in tracked:
        if j["a"] is j["b"]:
            assert np.all(np.abs(S) <= err) and Bnd.max() > 0
            n += 1
    assert n >= 3


def test_the_bound_is_small_against_the_scale_of_every_gpu_problem(tracked):
    worst = 0.0
    for L, k, j, S, err, Bnd in tracked:
        assert np.all(np.isfinite(S.astype(np.float64))) and np.all(err > 0)
        r = float(np.max(err / Bnd)); worst = max(worst, r)
        assert r <= 1e-10, (L["name"], k, r)
    print("%d relative jobs: largest bound / (|J| |P_s| |J|^T) %.3g" % (len(tracked), worst))


@pytest.mark.parametrize("mutation", ("sign", "swap", "plus3"))
def test_seeded_mutations_exceed_the_bound_on_every_problem_they_apply_to(tracked, mutation):
    """the sign of the [d]x term; a and b swapped in J only; position columns taken as theta + 3 on a split-column job"""
    n = 0; least = np.inf
    for L, k, j, S, err, Bnd in tracked:
        a, b = j["a"], j["b"]
        if a is b:
            continue                                      # (J [x; x] = 0 whatever J's blocks are)
        d = np.asarray(b[3]) - np.asarray(a[3])
        if mutation == "sign" and not np.any(d):
            continue
        if mutation == "plus3" and a[1] == a[0] + 3 and b[1] == b[0] + 3:
            continue
        r = float(np.max(np.abs(R.sigma(j, L["P"], mutate=mutation) - S) / err))
        least = min(least, r); n += 1
        assert r > 1.0, (L["name"], k, mutation, r)
    print("%s: %d problems, smallest |mutated - Sigma| / bound %.3g" % (mutation, n, least))
    assert n >= (5 if mutation == "plus3" else 100)


def test_relative_covariance_is_consistent_on_the_oracles_filter():
    """Sigma_rel of consecutive clones of the oracle's filter, after every message, against the simulation's trajectory at the clone
    times: d2 = e^T Sigma_rel^-1 e, six degrees of freedom; Sigma_rel symmetric and positive definite"""
    from oracle import lvo_be
    from tests import feature_sim as F
    sim = F.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)
    ekf = lvo_be.Ekf(sim["cfg"])
    d2 = []

    def on_update(ts):
        P = ekf.cov(); cl = ekf.clones()
        for i, S in enumerate(R.window_sigma(P, cl)):
            assert np.array_equal(S, S.T) or np.max(np.abs(S - S.T)) <= 1e-15 * np.abs(S).max()
            S = (S + S.T) / 2
            assert np.linalg.eigvalsh(S).min() > 0
            a, b = cl[i], cl[i + 1]
            d2.append(R.edge_d2(sim["traj"], a["time"], b["time"], a["q"], a["p"], b["q"], b["p"], S))
    n = F.drive(ekf, sim, on_update)
    d2 = np.array(d2)
    q = np.quantile(d2, [0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
    print("%d updates, %d edges; d2 = e^T Sigma_rel^-1 e: 10/25/50/75/90/99 %% = %s, share below %.2f: %.3f" % (n, len(d2), np.array2string(q, precision=3), R.CHI2_6_999,
                                                                                                                np.mean(d2 < R.CHI2_6_999)))
    assert n >= 40 and len(d2) > 200
    assert np.median(d2) < R.CHI2_6_999
