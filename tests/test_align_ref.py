"""CPU: the restatement tests/align_ref.py of the two-point alignment judged on its own - it recovers a planted alignment, its roots
satisfy the constraint they were solved from, its refinement ends at a stationary point - the cases of tests/align_cases.py meet the
conditions that make their discrete results well defined, a plain float64 run of the same definition agrees with the long-double one on
every discrete result, four seeded mistakes are each caught, and the library's pair drawing (host code) is the restatement's."""
import numpy as np
import pytest

from tests import align_cases as AC
from tests import align_ref as AR

LD = AR.LD


def _psi_err(c, s, psi):
    return float(np.arctan2(float(s) * np.cos(psi) - float(c) * np.sin(psi), float(c) * np.cos(psi) + float(s) * np.sin(psi)))


def test_noise_free_data_give_the_planted_alignment():
    for name in ("n63_clean_all_pairs", "planted_tie", "level_dz_zero_4"):
        k = AC.cases()[name]; r = AC.reference(name)
        psi, t = k["truth"]
        c, s, tt = r["model"]
        assert r["status"] == AR.OK and r["n_inliers"] == len(k["X"])
        assert abs(_psi_err(c, s, psi)) <= 1e-12 and np.abs(np.asarray(tt, np.float64) - t).max() <= 1e-12, name
        c0, s0, t0 = r["min_model"]
        assert abs(_psi_err(c0, s0, psi)) <= 1e-12 and np.abs(np.asarray(t0, np.float64) - t).max() <= 1e-12, name


def test_noisy_data_land_inside_five_sigma_of_the_normal_matrix():
    """24 matches, 8 of them wrong, 0.002 of noise, every pair; per seed the error of (psi, t) against 5 sqrt(diag(sigma^2 A^-1)).  With
    Gaussian noise and a threshold of five sigma the linearised covariance is right to first order and 5 sigma is passed once in 1.7
    million per component: the share of seeds inside must be at least 99 % (two of 200 may fail: wrong matches that slip in)."""
    sigma = 0.002; inside = 0; seeds = 200
    for sd in range(seeds):
        k = AC.scene(1000 + sd, 24, outliers=1 / 3, noise=sigma)
        r = AR.run(k["X"], k["uv"], AR.draw_pairs(24), k["R_wc"], k["p_wc"])
        if r["status"] != AR.OK:
            continue
        psi, t = k["truth"]
        c, s, tt = r["model"]
        e = np.array([_psi_err(c, s, psi), *(np.asarray(tt, np.float64) - t)])
        cov = sigma * sigma * np.linalg.inv(r["A"].astype(np.float64))
        inside += bool(np.all(np.abs(e) <= 5 * np.sqrt(np.diag(cov))))
    print("inside 5 sigma: %d of %d" % (inside, seeds))
    assert inside >= 0.99 * seeds


def test_both_roots_satisfy_the_two_point_constraint():
    """Rz (X_i - X_j) = l_i d_i - l_j d_j: with the model's t, Rz X + t - p_wc must lie ON the bearing of i and of j"""
    k = AC.cases()["n65_out70_all_pairs"]; r = AC.reference("n65_out70_all_pairs")
    d = np.concatenate([k["uv"], np.ones((len(k["uv"]), 1))], 1).astype(LD) @ k["R_wc"].astype(LD).T
    worst = 0.0; seen_two = 0
    for h in np.nonzero(r["n_models"])[0]:
        seen_two += r["n_models"][h] == 2
        for slot in range(r["n_models"][h]):
            c, s, t = r["c"][h, slot], r["s"][h, slot], r["t"][h, slot]
            for q in k["pairs"][h]:
                X = k["X"][q].astype(LD)
                g = np.array([c * X[0] - s * X[1], s * X[0] + c * X[1], X[2]], LD) + t - k["p_wc"].astype(LD)
                lam = (g @ d[q]) / (d[q] @ d[q])
                assert lam > 0
                worst = max(worst, float(np.abs(g - lam * d[q]).max() / np.abs(g).max()))
    assert seen_two >= 5 and worst <= 1e-12, (seen_two, worst)


def test_refinement_ends_at_a_stationary_point():
    for name in AC.cases():
        r = AC.reference(name)
        if r["status"] == AR.OK:
            assert np.all(np.abs(r["grad"].astype(np.float64)) <= 1e-10 * r["absg"] + r["gfloor"]), (name, r["grad"], r["absg"], r["gfloor"])
            assert 1 <= r["iters"] <= 10


def test_rz_is_orthonormal():
    for name in AC.cases():
        r = AC.reference(name)
        used = np.arange(2)[None, :] < r["n_models"][:, None]
        assert np.all(np.abs(r["c"][used] ** 2 + r["s"][used] ** 2 - 1) <= 8 * AR.U_LD), name
        c, s, _ = r["model"]
        assert abs(c * c + s * s - 1) <= 1e-15


@pytest.mark.parametrize("n", [2, 3, 91, 1024])
def test_library_draws_the_restatements_pairs(n):
    """host code of the library: runs without a GPU"""
    from larvio_amd import ops
    for mh, seed in ((0, 0), (0, 7), (4096, 0xFFFFFFFF), (5, 123456789), (4095, 1)):
        got = ops.align_draw_pairs(n, mh, seed); want = AR.draw_pairs(n, mh, seed)
        assert len(got) == len(want) == min(n * (n - 1) // 2, mh or 4096), (n, mh, seed)
        assert np.array_equal(np.stack([got["i"], got["j"]], 1).reshape(-1, 2), want), (n, mh, seed)
    assert np.array_equal(ops.align_draw_pairs(n, 0, 0)["i"], ops.align_draw_pairs(n, 0, 0xFFFFFFFF)["i"])      # a seed of 0 is the header's constant
    if n == 91:
        assert len(ops.align_draw_pairs(n)) == 4095                                                          # one under the cap: still every pair
    with pytest.raises(ValueError):
        ops.align_draw_pairs(n, 4097, 0)
    assert len(ops.align_draw_pairs(1)) == 0 and len(ops.align_draw_pairs(0)) == 0


@pytest.mark.parametrize("name", list(AC.cases()))
def test_case_meets_its_conditions_and_float64_agrees(name):
    k = AC.cases()[name]; r = AC.reference(name); f = AC.reference(name, "f64")
    low = {m: v for m, v in r["margins"].items() if v < AC.MARGIN and m not in AC.exempt(name)}
    assert not low, (name, low)
    assert not r["tie"] or "tie" in k["planted"], name
    assert AR.same_discrete(r, f) == [], name
    w = k["want"]
    for key in ("status", "hyp", "root_w", "n_inliers"):
        if key in w:
            assert r[key] == w[key], (name, key, r[key])
    for code in w.get("reasons", []):
        assert (r["reason"] == code).any(), (name, code)
    for flag in w.get("flags", []):
        assert r["flags"][flag].any(), (name, flag)
    if r["status"] == AR.OK and name not in ("n2_one_pair",):
        assert not r["mask"].astype(bool)[~k["good"]].any(), name                     # no wrong match among the winner's inliers


def _caught(name, mutate):
    """does the mistake change a discrete result of the case, or move a continuous one past its bound?"""
    k = AC.cases()[name]; r = AC.reference(name); b = AC.reference_bounds(name)
    with np.errstate(all="ignore"):
        m = AR.run(k["X"], k["uv"], k["pairs"], k["R_wc"], k["p_wc"], k["opt"], "ld", mutate=mutate)
    if AR.same_discrete(r, m):
        return True
    used = np.arange(2)[None, :] < r["n_models"][:, None]
    over = any(np.any(np.abs(m[f] - r[f])[used] > b[f][used]) for f in ("c", "s", "t"))
    got = np.array([m["model"][0], m["model"][1], *m["model"][2]], LD); want = np.array([r["model"][0], r["model"][1], *r["model"][2]], LD)
    return bool(over or np.any(np.abs(got - want) > b["model"]))


@pytest.mark.parametrize("mutate,names", [("sign_s", ["n65_out70_all_pairs", "n64_out30_4", "planted_tie", "n2_one_pair"]),
                                          ("transpose", ["n65_out70_all_pairs", "n64_out30_4", "n1024_out30_5"]),
                                          ("small_dz", ["level_dz_zero_4"]),      # (elsewhere it is the same solver, only worse conditioned)
                                          ("tie_high", ["planted_tie", "n63_clean_all_pairs", "level_dz_zero_4"])])
def test_seeded_mistake_is_caught(mutate, names):
    for name in names:
        assert _caught(name, mutate), (mutate, name)
