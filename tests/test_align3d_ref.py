"""CPU: the restatement tests/align3d_ref.py of the 3D-3D alignment (lvk_align_ransac_3d) judged on its own, and the numpy mirrors in
larvio_amd/localize.py (align_points, invert_alignment, transform_points, merge_maps).

- no case of tests/align3d_cases.py has a deciding comparison inside the first-order error bound its float64 evaluation carries (the
  solver's four comparisons, every inlier test, the SINGULAR test; the arg-max compares the integer counts those tests give) - so the
  discrete results are the same in any arithmetic, and a plain float64 run agrees with the long-double one on every one of them;
- localize.align_points is that float64 run bit for bit in everything discrete and in every hypothesis, and inside the bound in the
  refined model;
- A is the normal matrix of the residual (central differences), the closed form is where Gauss-Newton from the winner ends;
- invert_alignment undoes an alignment on random points, and is lvk_align_invert (host code of the library) bit for bit;
- merge_maps on two synthetic sessions keeps the right set and finds the generating alignment inside the refinement's bound plus the
  noise's own term; seeded mistakes are caught."""
import numpy as np
import pytest

from larvio_amd import localize as L
from tests import align3d_cases as C3
from tests import align3d_ref as R3

LD = R3.LD


P_FALSE = 1e-6          # the chance that a right model fails a truth check below, over all the components it compares


def _noise_bound(A, sigma, n_comp=4, p=P_FALSE):
    """What Gaussian noise of `sigma` per coordinate on the inliers may move (psi, t_x, t_y, t_z) by: their covariance is sigma^2 A^-1 (A
    the refinement's normal matrix; for t about the centroid its diagonal is sigma^2 / n), and the two-sided normal quantile that all
    n_comp components stay inside with probability 1 - p (a union bound: p / n_comp each) is the multiplier - 5.16 for four components
    and one in a million.  -> (the bound per component, the multiplier)"""
    from statistics import NormalDist
    k = NormalDist().inv_cdf(1.0 - p / (2.0 * n_comp))
    return k * sigma * np.sqrt(np.diag(np.linalg.inv(np.asarray(A, np.float64)))), k


def _psi_err(c, s, psi):
    return float(np.arctan2(float(s) * np.cos(psi) - float(c) * np.sin(psi), float(c) * np.cos(psi) + float(s) * np.sin(psi)))


@pytest.mark.parametrize("name", list(C3.cases()))
def test_case_has_no_decision_inside_its_margin_and_float64_agrees(name):
    k = C3.cases()[name]; r = C3.reference(name); f = C3.reference(name, "f64")
    print(name, "flagged comparisons:", C3.flagged(name))
    assert C3.flagged(name) == 0, name
    assert R3.same_discrete(r, f) == [], name
    w = k["want"]
    for key in ("status", "hyp", "n_inliers", "tie"):
        if key in w:
            assert r[key] == w[key], (name, key, r[key])
    if "n_pairs" in w:
        assert len(k["pairs"]) == w["n_pairs"]
    for code in w.get("reasons", []):
        assert (r["reason"] == code).any(), (name, code)
    if "reason_list" in w:
        assert r["reason"].tolist() == w["reason_list"], name
    if r["status"] == R3.OK:
        assert not r["mask"].astype(bool)[~k["good"]].any(), name                     # no wrong match among the winner's inliers
        psi, t = k["truth"]
        c, s, tt = r["model"]
        err = np.abs(np.array([_psi_err(c, s, psi), *(np.asarray(tt, np.float64) - t)]))
        if k["noise"] == 0:                                                             # exact data: what is left is rounding, of numbers below 32
            assert err.max() <= 1e-12, (name, err)
        else:                                                                           # the case's own noise through its own normal matrix
            tol, mult = _noise_bound(r["A"], k["noise"])
            print(name, "truth error / (sigma sqrt(diag A^-1)):", err / (tol / mult), "allowed", mult)
            assert np.all(err <= tol), (name, err, tol)
        assert abs(float(c * c + s * s) - 1.0) <= 1e-15


def test_the_table_covers_what_it_must_and_flags_nothing():
    names = list(C3.cases())
    assert sum(C3.flagged(n) for n in names) == 0                                       # over the WHOLE table: no case is left out
    st = {n: C3.reference(n)["status"] for n in names}
    assert {R3.OK, R3.NO_MODEL, R3.FEW_INLIERS, R3.SINGULAR} == set(st.values())
    assert {len(C3.cases()[n]["X"]) for n in names} >= {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1024}
    assert {len(C3.cases()[n]["pairs"]) for n in names} >= {0, 1, 64, 4095, 4096}
    reasons = np.concatenate([C3.reference(n)["reason"] for n in names if len(C3.cases()[n]["X"]) >= 2])
    assert set(reasons.tolist()) == {R3.R_MODEL, R3.R_INDEX, R3.R_RHO, R3.R_DZ, R3.R_LENGTH}
    assert any(C3.reference(n)["tie"] for n in names)
    # exhaustive against drawn at the boundary: 91 matches have exactly 4095 pairs, each once; 92 are drawn with the generator
    p91 = C3.cases()["n91_out30_exhaustive_4095"]["pairs"]; p92 = C3.cases()["n92_out30_drawn_4096"]["pairs"]
    assert len(set(map(tuple, p91.tolist()))) == 4095 and (p91[:, 0] < p91[:, 1]).all()
    assert len(p92) == 4096 and (p92[:, 0] > p92[:, 1]).any()


@pytest.mark.parametrize("name", list(C3.cases()))
def test_localize_align_points_is_the_float64_restatement(name):
    k = C3.cases()[name]; f = C3.reference(name, "f64"); r = C3.reference(name); b = C3.reference_bounds(name)
    g = L.align_points(k["X"], k["Y"], k["pairs"], **k["opt"])
    assert g["status"] == f["status"] and g["hyp"] == f["hyp"] and g["n_inliers"] == f["n_inliers"] and np.array_equal(g["mask"], f["mask"])
    assert np.array_equal(g["n_models"], f["n_models"]) and np.array_equal(g["count"], f["count"])
    for a, bb in ((g["hc"], f["c"]), (g["hs"], f["s"]), (g["ht"], f["t"])):
        assert np.asarray(a, np.float64).tobytes() == np.asarray(bb, np.float64).tobytes(), name
    assert np.array([g["c0"], g["s0"], *g["t0"]]).tobytes() == np.array([f["min_model"][0], f["min_model"][1], *f["min_model"][2]], np.float64).tobytes()
    got = np.array([g["c"], g["s"], *g["t"]], LD); want = np.array([r["model"][0], r["model"][1], *r["model"][2]], LD)
    if r["status"] == R3.OK:
        assert np.all(np.abs(got - want) <= b["model"]), (name, np.abs(got - want), b["model"])
    assert np.all(np.abs(g["A"].astype(LD) - r["A"]) <= b["A"]) and abs(LD(g["rms"]) - r["rms"]) <= b["rms"], name


@pytest.mark.parametrize("name", ["n64_out30_64", "n257_out60_64", "n2_one_pair"])
def test_A_is_the_normal_matrix_of_the_residual_by_central_differences(name):
    k = C3.cases()[name]; r = C3.reference(name)
    sel = r["mask"].astype(bool)
    X = k["X"][sel].astype(LD); Y = k["Y"][sel].astype(LD)
    c, s, t = r["model"]
    psi0 = np.arctan2(LD(s), LD(c))

    def resid(p):
        cc, ss = np.cos(p[0]), np.sin(p[0])
        return np.stack([cc * X[:, 0] - ss * X[:, 1] + p[1] - Y[:, 0], ss * X[:, 0] + cc * X[:, 1] + p[2] - Y[:, 1], X[:, 2] + p[3] - Y[:, 2]], -1).reshape(-1)
    p0 = np.array([psi0, *t], LD); h = LD(1e-6)
    J = np.stack([(resid(p0 + h * e) - resid(p0 - h * e)) / (2 * h) for e in np.eye(4, dtype=LD)], -1)
    A = J.T @ J
    assert np.abs(A - r["A"]).max() <= 1e-9 * np.abs(r["A"]).max(), name                # the differences' own truncation: h^2 / 6 of a third derivative
    assert abs(np.sqrt((resid(p0) ** 2).sum() / sel.sum()) - r["rms"]) <= 1e-15


@pytest.mark.parametrize("name", ["n64_out30_64", "n65_out60_all_pairs", "n255_out80_4096", "n2_one_pair"])
def test_closed_form_is_where_gauss_newton_from_the_winner_ends(name):
    k = C3.cases()[name]; r = C3.reference(name)
    sel = r["mask"].astype(bool)
    c0, s0, t0 = r["min_model"]
    c, s, t = R3.gauss_newton(c0, s0, t0, k["X"][sel], k["Y"][sel])
    cm, sm, tm = r["model"]
    assert abs(c - cm) <= 1e-13 and abs(s - sm) <= 1e-13 and np.abs(t - tm).max() <= 1e-12, name


def test_invert_alignment_round_trip_and_the_librarys_host_code():
    from larvio_amd import ops
    rng = np.random.default_rng(5)
    for _ in range(20):
        psi = rng.uniform(-np.pi, np.pi); t = rng.uniform(-50, 50, 3)
        al = dict(c=np.cos(psi), s=np.sin(psi), t=t)
        ci, si, ti = L.invert_alignment(al)
        X = rng.uniform(-100, 100, (50, 3))
        Yp, _ = L.apply_alignment(al, X)
        back, _ = L.apply_alignment(dict(c=ci, s=si, t=ti), Yp)
        assert np.abs(back - X).max() <= 64 * 2.0 ** -53 * 400                          # a few roundings of numbers below 400
        rec = ops.align_invert((al["c"], al["s"], al["t"]))
        assert np.array([rec["c"], rec["s"], *rec["t"]]).tobytes() == np.array([ci, si, *ti]).tobytes()
        assert rec["status"] == 0 and not rec["A"].any() and rec["c0"] == 0 and rec["rms"] == 0
        p1, _ = L.transform_points(X, None, al)
        assert p1.tobytes() == Yp.tobytes()                                              # transform_points' p is apply_alignment's


def test_transform_points_rotates_the_covariance_and_adds_the_alignments():
    rng = np.random.default_rng(6)
    X = rng.uniform(-20, 20, (40, 3)); M = rng.normal(size=(40, 3, 3)); cov = M @ M.transpose(0, 2, 1)
    psi = 0.9; al = dict(c=np.cos(psi), s=np.sin(psi), t=np.array([1.0, 2.0, 3.0]))
    Q = rng.normal(size=(4, 4)); P = 1e-4 * (Q @ Q.T)
    p, w = L.transform_points(X, cov, al, P)
    Rz = np.array([[al["c"], -al["s"], 0], [al["s"], al["c"], 0], [0, 0, 1.0]])
    q = X @ Rz.T
    J = np.zeros((40, 3, 4)); J[:, 0, 0] = -q[:, 1]; J[:, 1, 0] = q[:, 0]; J[:, 0, 1] = J[:, 1, 2] = J[:, 2, 3] = 1
    want = Rz @ cov @ Rz.T + J @ P @ J.transpose(0, 2, 1)
    assert np.abs(w - want).max() <= 1e-12 * np.abs(want).max() and np.array_equal(w, w.transpose(0, 2, 1))
    _, only = L.transform_points(X, None, al, P)
    assert np.abs(only - J @ P @ J.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(want).max()
    pi, wi = L.transform_points(X, cov, None)
    assert pi.tobytes() == (X + 0.0).tobytes() and np.abs(wi - cov).max() <= 1e-12 * np.abs(cov).max()


def _merge_expectation(S):
    """the kept set by reasoning alone: every point of A and B once, of a point seen twice the copy with the smaller covariance trace"""
    (XA, covA, dA), (XB, covB, dB) = S["A"], S["B"]
    nA, nS = len(XA), len(S["shared"])
    trA = np.trace(covA, axis1=1, axis2=2); trB = np.trace(covB, axis1=1, axis2=2)
    keep = set(range(nA)) | set(nA + np.arange(len(XB)))
    for r, a in enumerate(S["shared"]):
        keep.discard(int(a) if trB[r] < trA[a] else nA + r)
    return keep


def test_merge_maps_keeps_the_right_set_and_finds_the_generating_alignment():
    S = C3.sessions(); P = C3.SESSIONS
    m = L.merge_maps(S["A"], S["B"], r_dup=P["r_dup"], seed=7)
    al = m["align"]
    assert m["merged"] and al["status"] == R3.OK
    good = (m["matches"][:, 0] >= 0)
    assert al["n_inliers"] >= 100 and int(m["match_info"]["n_selected"]) >= P["n_shared"] - 5 and good.all()
    # the alignment against the truth: the refinement's V-carried bound plus the noise's own term (_noise_bound: sigma^2 A^-1, the
    # multiplier from the number of components compared and a stated chance of a false failure)
    Xs, Ys = m["matches_X"], m["matches_Y"]
    ref = R3.run(Xs, Ys, m["pairs"], None, "ld")
    bnd = R3.bounds(Xs, Ys, m["pairs"], ref)
    noise, mult = _noise_bound(al["A"], P["sigma"])
    psi, t = S["truth"]
    err = np.array([_psi_err(al["c"], al["s"], psi), *(np.asarray(al["t"]) - t)])
    tol = noise + np.array([float(bnd["model"][0] + bnd["model"][1]), *[float(x) for x in bnd["model"][2:]]])
    print("alignment error", err, "bound", tol, "error / (sigma sqrt(diag A^-1))", np.abs(err) / (noise / mult), "allowed", mult)
    assert np.all(np.abs(err) <= tol), (err, tol)
    # t_z does not couple with the yaw: its term is exactly the multiplier times sigma / sqrt(n)
    assert abs(noise[3] - mult * P["sigma"] / np.sqrt(al["n_inliers"])) <= 1e-12 * noise[3]
    # the kept set, and the order's two halves
    nA = P["n_a"]
    assert set(m["order"].tolist()) == _merge_expectation(S) and len(m["order"]) == nA + P["n_new"] == int(m["info"]["n_kept"])
    assert int(m["info"]["n_duplicate"]) == P["n_shared"]
    tr = np.trace(m["cov"], axis1=1, axis2=2)
    assert np.all(np.diff(tr) >= 0)                                                      # best first
    fromA = m["order"] < nA
    assert np.array_equal(m["X"][fromA], S["A"][0][m["order"][fromA]]) and np.array_equal(m["desc"][~fromA], S["B"][2][m["order"][~fromA] - nA])
    # B's points landed where A has them
    back = {int(a): r for r, a in enumerate(S["shared"])}
    for pos in np.nonzero(~fromA)[0]:
        r = int(m["order"][pos]) - nA
        if r < P["n_shared"]:
            assert np.abs(m["X"][pos] - S["A"][0][S["shared"][r]]).max() <= 6 * P["sigma"]
    assert len(back) == P["n_shared"]


def test_merge_maps_with_a_given_alignment_and_without_overlap():
    S = C3.sessions(); P = C3.SESSIONS
    psi, t = S["truth"]
    fwd = dict(c=np.cos(-psi), s=np.sin(-psi), t=-(np.array([[np.cos(psi), np.sin(psi), 0], [-np.sin(psi), np.cos(psi), 0], [0, 0, 1.0]]) @ t))     # A -> B
    ci, si, ti = L.invert_alignment(fwd)
    m = L.merge_maps(S["A"], S["B"], align=dict(c=ci, s=si, t=ti), r_dup=P["r_dup"])
    assert m["merged"] and m["match_info"] is None and set(m["order"].tolist()) == _merge_expectation(S)
    far = (S["B"][0][P["n_shared"]:], S["B"][1][P["n_shared"]:], S["B"][2][P["n_shared"]:])      # only B's new points: nothing to find
    m = L.merge_maps(S["A"], far, r_dup=P["r_dup"])
    assert not m["merged"] and m["align"]["status"] != R3.OK and m["order"] is None


@pytest.mark.parametrize("mutate,names", [("sign_s", ["n64_out30_64", "n2_one_pair", "planted_tie"]), ("tie_high", ["planted_tie", "n63_clean_all_pairs"]),
                                          ("no_z", ["refused_by_each_rule"])])
def test_seeded_mistake_is_caught(mutate, names):
    for name in names:
        k = C3.cases()[name]; r = C3.reference(name)
        with np.errstate(all="ignore"):
            m = R3.run(k["X"], k["Y"], k["pairs"], k["opt"], "ld", mutate=mutate)
        assert R3.same_discrete(r, m), (mutate, name)
