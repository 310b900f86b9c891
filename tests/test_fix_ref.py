"""The restatement the GPU tests of lvk_ekf_update_sparse and lvk_ekf_add_fix compare against (tests/fix_ref.py), held to itself on the
CPU: the closed-form H of both measurement models against central differences of the prediction under the filter's injection, the
update against numpy.linalg's K = P H^T S^-1, the zero covariance, the whitened-rows form update_zupt uses, the distance of every
problem's gamma from its gate, the size of the derived bound and its power to tell four seeded mistakes from the truth on every problem
of the GPU stage tests they apply to."""
import numpy as np
import pytest

from tests import fix_ref as F

LD = F.LD


@pytest.fixture(scope="module")
def tracked():
    """(problem, update_tracked(problem)) of every problem of the GPU stage tests, computed once"""
    return [(pr, F.update_tracked(pr["P"], pr["cols"], pr["H"], pr["r"], pr["R"], pr["gate"])) for pr in F.stage_problems()]


def _model_problems():
    return [pr for pr in F.stage_problems() if not pr["generic"]]


def test_the_problems_cover_what_the_issue_lists():
    ps = F.stage_problems()
    assert {p["n"] for p in ps} == {28, 34, 63, 64, 65, 433}
    assert {p["ldp"] - p["n"] for p in ps} == {0, F.PAD}
    assert {p["H"].shape[0] for p in ps} == {3, 6} and {p["H"].shape[1] for p in ps} == {3, 6, 12}
    assert any(list(p["cols"]) == [0, 1, 2] for p in ps) and any(list(p["cols"][-6:]) == list(range(p["n"] - 6, p["n"])) for p in ps)
    assert {p["a"] for p in ps if p["H"].shape[1] == 12 and not p["generic"]} >= {0.0, 0.5, 1.0}
    assert {bool(np.any(p["lever"])) for p in ps if not p["generic"]} == {False, True}


def test_closed_form_H_equals_the_central_difference_H():
    worst = 0.0; n = 0
    for pr in _model_problems():
        _, H, _ = F.fix_rows(pr["kind"], pr["poses"], pr["a"], pr["lever"], pr["z_p"], pr["z_q"])
        H_nd = F.jacobian_nd(pr["kind"], pr["poses"], pr["a"], pr["lever"])
        scale = 1 + float(np.linalg.norm(pr["lever"]))
        worst = max(worst, float(np.max(np.abs(H_nd - H.v))) / scale); n += 1
        assert np.any(H.v != 0)
    print("%d problems: largest |H_nd - H_closed| / (1 + |l|) = %.2e (TOL_ND %.0e)" % (n, worst, F.TOL_ND))
    assert n >= 10 and worst < F.TOL_ND


def test_residual_is_the_measurement_minus_the_prediction_and_vanishes_on_it():
    for pr in _model_problems():
        z_p = F.predict_position(pr["poses"], pr["a"], pr["lever"]).astype(np.float64)
        _, _, r = F.fix_rows(pr["kind"], pr["poses"], pr["a"], pr["lever"], z_p, pr["poses"][0][1])
        assert np.max(np.abs(r.v)) < 1e-14 and np.all(np.abs(r.v) <= 2 * r.e + 1e-15)      # (z_p was rounded to float64)
        # a small injected error is read back by the residual: r = H delta to first order
        d = np.zeros(6 * len(pr["poses"]), LD); d[:] = 1e-6 * np.arange(1, len(d) + 1)
        deltas = [d[6 * s:6 * s + 6] for s in range(len(pr["poses"]))]
        zp = F.predict_position(pr["poses"], pr["a"], pr["lever"], deltas)
        zq = F.inject(pr["poses"][0][1], pr["poses"][0][2], deltas[0])[0]
        _, H, r = F.fix_rows(pr["kind"], pr["poses"], pr["a"], pr["lever"], zp.astype(np.float64), zq.astype(np.float64))
        assert np.max(np.abs(r.v - H.v @ d)) < 1e-10


def test_restatement_against_numpy_linalg(tracked):
    """float64 numpy.linalg: K = P H^T S^-1, dx = K r, P' = P - K S K^T with a dense H.  Its own rounding is of the order u cond(S) times
    the scale of the result - cond(S) <= 1e10 by construction (variances 1e-8 .. 1e2 and R >= 2.5e-3) gives 1e-6, times a modest
    constant: 1e-5, norm-wise - far below what a wrong formula would do"""
    n = 0
    for pr, t in tracked:
        if t["status"] != 0:
            continue
        P = pr["P"]; Hd = np.zeros((pr["H"].shape[0], pr["n"])); Hd[:, pr["cols"]] = pr["H"]
        S = Hd @ P @ Hd.T + pr["R"]
        K = np.linalg.solve(S, Hd @ P).T
        dx = K @ pr["r"]; Pn = P - K @ S @ K.T
        g = float(pr["r"] @ np.linalg.solve(S, pr["r"]))
        assert np.max(np.abs(dx - t["dx"])) <= 1e-5 * np.max(np.abs(dx)), pr["name"]
        assert np.max(np.abs(Pn - t["P"])) <= 1e-5 * np.max(np.abs(P)), pr["name"]
        assert abs(g - float(t["gamma"])) <= 1e-5 * g, pr["name"]
        plain = F.update(P, pr["cols"], pr["H"], pr["r"], pr["R"], pr["gate"])
        assert np.all(np.abs(plain["dx"] - t["dx"]) <= t["e_dx"]) and np.all(np.abs(plain["P"] - t["P"]) <= t["e_P"])
        n += 1
    assert n >= 12


def test_zero_covariance_gives_zero_dx_and_leaves_P(tracked):
    for pr, _ in tracked:
        Z = np.zeros_like(pr["P"])
        t = F.update_tracked(Z, pr["cols"], pr["H"], pr["r"], pr["R"], 0.0)
        assert t["status"] == 0 and np.all(t["dx"] == 0) and np.all(t["P"] == 0) and np.all(t["e_dx"] == 0) and np.all(t["e_P"] == 0)
        p = F.update(Z, pr["cols"], pr["H"], pr["r"], pr["R"])
        assert np.all(p["dx"] == 0) and np.all(p["P"] == 0)


def test_agreement_with_the_whitened_rows_form_of_update_zupt(tracked):
    """the same update through rows whitened to an isotropic sigma2 and the dense form: another order of operations in the same long
    double, so the two differ by this file's rounding only - inside the bound derived for float64, with room"""
    worst = 0.0; n = 0
    for pr, t in tracked:
        if t["status"] != 0 or pr["n"] > 100:
            continue
        dx, Pn = F.whitened_update(pr["P"], pr["cols"], pr["H"], pr["r"], pr["R"])
        w = max(float(np.max(np.abs(dx - t["dx"]) / t["e_dx"])), float(np.max(np.abs(Pn - t["P"]) / t["e_P"])))
        assert w <= 1.0, (pr["name"], w)
        worst = max(worst, w); n += 1
    print("whitened rows: %d problems, largest |difference| / bound %.3g" % (n, worst))
    assert n >= 8
    # diagonal R: the scaling update_zupt writes, sqrt(sigma2 / R_ii) per row
    pr = F.stage_problems()[0]; Rd = np.diag(np.diag(pr["R"]))
    s2 = LD(6.4e-5); s = np.sqrt(s2 / np.diag(Rd).astype(LD))
    Hd = np.zeros((3, pr["n"]), LD); Hd[:, pr["cols"]] = pr["H"]; Hw = Hd * s[:, None]; rw = pr["r"] * s
    P = pr["P"].astype(LD)
    L = F.chol(Hw @ P @ Hw.T + s2 * np.eye(3, dtype=LD)); W = F.fsub(L, Hw @ P)
    t = F.update_tracked(pr["P"], pr["cols"], pr["H"], pr["r"], Rd)
    assert np.all(np.abs(W.T @ F.fsub(L, rw) - t["dx"]) <= t["e_dx"]) and np.all(np.abs(P - W.T @ W - t["P"]) <= t["e_P"])


def test_no_problem_has_gamma_near_its_gate_and_both_outcomes_occur(tracked):
    st = []
    for pr, t in tracked:
        assert t["status"] in (0, 1)
        if pr["gate"] > 0:
            assert abs(float(t["gamma"]) - pr["gate"]) > 1e-6 * pr["gate"], pr["name"]
            assert float(t["e_gamma"]) < 1e-6 * pr["gate"]
        st.append((pr["gate"] > 0, t["status"]))
    assert (True, 1) in st and (True, 0) in st and (False, 0) in st
    assert sum(s == 1 for _, s in st) == 2


def test_the_bound_is_small_against_the_scale_of_every_gpu_problem(tracked):
    worst = 0.0
    for pr, t in tracked:
        if t["status"] != 0:
            continue
        assert np.all(np.isfinite(t["P"].astype(np.float64))) and np.all(t["e_dx"] >= 0)
        r = max(float(np.max(t["e_P"]) / np.max(np.abs(t["P"]))), float(np.max(t["e_dx"]) / np.max(np.abs(t["dx"]))))
        worst = max(worst, r)
        assert r <= 1e-6, (pr["name"], r)          # u cond(S) k: 1.1e-16 * 1e10 * a few
    print("largest bound / scale %.3g" % worst)


@pytest.mark.parametrize("mutation", ("sign", "swap_a", "no_R", "swap_cols"))
def test_seeded_mistakes_exceed_the_bound_on_every_problem_they_apply_to(tracked, mutation):
    """the sign of [R l]x; a and 1 - a swapped; R left out of S; the d_theta and d_p columns swapped"""
    n = 0; least = np.inf
    for pr, t in tracked:
        if t["status"] != 0:
            continue
        H, r = pr["H"], pr["r"]
        if mutation in ("sign", "swap_a"):
            if pr["generic"] or (mutation == "sign" and not np.any(pr["lever"])) or (mutation == "swap_a" and (len(pr["poses"]) < 2 or pr["a"] == 0.5)):
                continue
            _, Hm, rm = F.fix_rows(pr["kind"], pr["poses"], pr["a"], pr["lever"], pr["z_p"], pr["z_q"], mutate=mutation)
            H, r = Hm.v, rm.v
        if mutation == "swap_cols" and len(pr["cols"]) % 6:
            continue
        bad = F.update(pr["P"], pr["cols"], H, r, pr["R"], mutate=mutation if mutation in ("no_R", "swap_cols") else None)
        ratio = max(float(np.max(np.abs(bad["dx"] - t["dx"]) / t["e_dx"])), float(np.max(np.abs(bad["P"] - t["P"]) / np.where(t["e_P"] > 0, t["e_P"], np.inf))))
        least = min(least, ratio); n += 1
        assert ratio > 1.0, (pr["name"], mutation, ratio)
    print("%s: %d problems, smallest |mutated - truth| / bound %.3g" % (mutation, n, least))
    assert n >= {"sign": 5, "swap_a": 3, "no_R": 12, "swap_cols": 9}[mutation]
