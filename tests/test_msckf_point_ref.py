"""The restatement the GPU tests of lvk_ekf_msckf_point_cov compare against (tests/msckf_point_ref.py), held to itself on the CPU: its
closed-form Jacobians against central differences of the projection written from the geometry, two closed forms of Sigma, the
conditioning of every problem the GPU tests use, and the size of the derived bound."""
import numpy as np
import pytest

from tests import msckf_point_ref as R

LD = R.LD


def _cases():
    rng = np.random.default_rng(7)
    clones = R.make_clones(rng, 20)
    out = []
    for M, leg, td, fej in ((2, 22, 0, 0), (3, 46, 1, 0), (7, 22, 1, 1), (16, 46, 0, 1)):
        n_cl = 20 if leg == 22 else 16
        ranks = rng.permutation(rng.choice(n_cl, M, replace=False))
        out.append(R.make_problem(rng, clones, ranks, leg_dim=leg, if_fej=fej, estimate_td=td))
    return out


CASES = _cases()


@pytest.mark.parametrize("k", range(len(CASES)))
def test_analytic_B_equals_the_central_difference_B(k):
    pr = CASES[k]
    n = pr["leg_dim"] + 6 * 20
    _, B_nd, _, _ = R.sigma_nd(pr, np.zeros((n, n)))
    B_an = R.B_tracked(pr)
    # scale: |G_t| |Hc_t| summed entrywise, from the analytic route
    H = [tuple(m.v for m in R.jacobians_tracked(pr["clones"][r], pr["p_w"], pr["if_fej"])) for r in pr["ranks"]]
    Habs = [(np.abs(a), np.abs(b), c) for a, b, c in H]
    A = sum(c.T @ c for _, _, c in H); Ainv = R.inv3(A)
    scale = np.zeros_like(B_an)
    for t, (ax, ae, hf) in enumerate(Habs):
        G = np.abs(Ainv @ hf.T)
        scale[:, 0:6] += G @ ae; scale[:, 6] += G @ np.abs(pr["zv"][t]).astype(LD); scale[:, 7 + 6 * t:13 + 6 * t] = G @ ax
    worst = float(np.max(np.abs(B_an - B_nd) / scale))
    print("M %d: |B_analytic - B_nd| / scale = %.2e (TOL_ND %.0e)" % (len(pr["ranks"]), worst, R.TOL_ND))
    assert worst < R.TOL_ND
    if not pr["estimate_td"]:
        assert np.all(B_an[:, 6] == 0) and np.all(B_nd[:, 6] == 0)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_zero_state_covariance_leaves_the_pixel_noise_term(k):
    pr = CASES[k]
    n = pr["leg_dim"] + 6 * 20
    S, err, Bnd, _ = R.sigma_tracked(pr, np.zeros((n, n)))
    Snd, _, Ainv, _ = R.sigma_nd(pr, np.zeros((n, n)))
    assert np.array_equal(Snd, LD(pr["sigma2"]) * Ainv)
    assert np.max(np.abs(S - Snd) / Bnd) < R.TOL_ND


@pytest.mark.parametrize("fej", (0, 1))
@pytest.mark.parametrize("k", range(len(CASES)))
def test_common_position_error_adds_s2_identity(k, fej):
    """position blocks of all observing clones at s2 I, fully correlated: every Hx_t position block is -Hf_t, so the position columns
    of B sum to -I and Sigma = sigma2 A^-1 + s2 I, with and without first-estimate Jacobians"""
    pr = dict(CASES[k]); pr["if_fej"] = bool(fej)
    n = pr["leg_dim"] + 6 * 20; s2 = 2.5e-3
    P = R.correlated_position_cov(n, pr["ranks"], pr["leg_dim"], s2)
    H = [tuple(m.v for m in R.jacobians_tracked(pr["clones"][r], pr["p_w"], pr["if_fej"])) for r in pr["ranks"]]
    zero = np.zeros((7 + 6 * len(H), 7 + 6 * len(H)), LD)
    # each route against its own A^-1: long-double rounding (u_ld cond(A), cond(A) < 1e6) for the closed forms, the differentiation
    # error on top for the central differences
    for S, Ainv, tol in ((R.sigma_tracked(pr, P)[0], R.assemble(H, pr["zv"], pr["estimate_td"], zero, 0.0)[2], 1e-13), (R.sigma_nd(pr, P)[0], R.sigma_nd(pr, 0 * P)[2], R.TOL_ND)):
        want = LD(pr["sigma2"]) * Ainv + LD(s2) * np.eye(3, dtype=LD)
        assert np.max(np.abs(S - want) / np.abs(want).max()) < tol


def test_every_gpu_problem_is_well_conditioned_and_its_bound_is_small():
    """cond(A) <= 1e6 for every problem the GPU stage tests use: none is left out of the comparison there.  The derived bound stays
    far below the quantity itself (1e-7 of the entrywise scale), so it cannot pass a wrong kernel."""
    worst_c = 0.0; worst_b = 0.0
    for L in R.stage_launches():
        for pr in L["probs"]:
            S, err, Bnd, cond = R.sigma_tracked(pr, L["P"])
            assert cond <= 1e6, (L["name"], cond)
            assert np.all(np.isfinite(S.astype(np.float64))) and np.all(err > 0)
            worst_c = max(worst_c, cond); worst_b = max(worst_b, float(np.max(err / Bnd)))
            assert np.all(np.linalg.eigvalsh(S.astype(np.float64)) > 0)
    print("largest cond(A) %.3g, largest bound / Bnd %.3g" % (worst_c, worst_b))
    assert worst_b < 1e-7


def test_degenerate_problem_has_an_exactly_zero_pivot():
    pr = R.degenerate_problem()
    H = [R.jacobians_tracked(pr["clones"][r], pr["p_w"], 0)[2].v.astype(np.float64) for r in pr["ranks"]]
    A = sum(h.T @ h for h in H)
    assert np.array_equal(A, np.diag([4 / 16.0, 4 / 16.0, 0.0]))
    assert R.ldl3(A)[1][2] == 0.0
