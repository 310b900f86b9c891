"""CPU: the restatement of lvk_map_select_queries (tests/map_select_ref.py) on every case of tests/map_select_cases.py, held to a plain
Python loop (the selection), to a long-double judge (pixel and radius: equal or adjacent float32; the margins that give the discrete
fields one right value), to larvio_amd.localize.predict_pixels (the VISIBLE set and the pixels), to the radius' closed form and to the
hand-written fields of the edge cases; and larvio_amd.localize.view_limit / map_obs."""
import numpy as np
import pytest

from larvio_amd import localize
from larvio_amd._lib import MAP_MATCH, MATCH_OK, ALIGN_RESULT
from tests import map_select_cases as MC
from tests import map_select_ref as R

NAMES = list(MC.cases())


@pytest.mark.parametrize("name", NAMES)
def test_selection_equals_the_plain_loop(name):
    k = MC.cases()[name]; ref = MC.reference(name); pr = ref["proj"]; o = k["o"]
    n = len(k["X"])
    step = 1 if n <= 5000 else 14                        # the loop is cells x points: the large case is thinned, the rule is the same
    st, cell = pr["status"][::step], pr["cell"][::step]
    nc = o["rows"] * o["cols"]
    assert np.array_equal(R.select(st, cell, nc, o["quota"]), R.select_loop(st, cell, nc, o["quota"]))
    idx = ref["sel"]["index"]
    assert np.array_equal(idx, R.select(pr["status"], pr["cell"], nc, o["quota"])) and ref["info"]["n_selected"] == len(idx) <= nc * o["quota"]
    key = ref["sel"]["cell"].astype(np.int64) * (n + 1) + idx
    assert (np.diff(key) > 0).all()                      # ordered by (cell, index)
    assert int(ref["info"]["n_visible"]) + int(ref["info"]["n_behind"]) + int(ref["info"]["n_far"]) + int(ref["info"]["n_outside"]) == n
    assert ((ref["status"] & R.SELECTED) != 0).sum() == len(idx) and ((ref["status"][idx] & 0x7F) == R.VISIBLE).all()
    if "index" in k["want"]:
        assert idx.tolist() == k["want"]["index"]
    if "status" in k["want"]:
        assert (ref["status"] & 0x7F).tolist() == k["want"]["status"]
    if "last_radius" in k["want"]:
        assert ref["sel"]["radius"][ref["sel"]["index"] == n - 1] == np.float32(k["want"]["last_radius"])


@pytest.mark.parametrize("name", NAMES)
def test_margins_and_the_long_double_judge(name):
    k = MC.cases()[name]; ref = MC.reference(name); j = MC.judged(name)
    if not k["exact"]:
        assert not MC.too_close(j, k["cam"], k["o"]).any()                     # every threshold is at least a margin away ...
    assert np.array_equal(j["status"], ref["proj"]["status"]) and np.array_equal(j["cell"], ref["proj"]["cell"])      # ... so both arithmetics agree
    idx = ref["sel"]["index"]
    for f in ("x", "y", "radius"):
        assert R.adjacent_or_equal(ref["sel"][f], j[f][idx]).all(), f
    assert ref["sel"]["depth"].tobytes() == np.asarray(j["depth"][idx]).astype(np.float32).tobytes() or R.adjacent_or_equal(ref["sel"]["depth"], np.asarray(j["depth"][idx]).astype(np.float32)).all()
    assert ((ref["sel"]["radius"] >= np.float32(k["o"]["r_min"])) & (ref["sel"]["radius"] <= np.float32(k["o"]["r_max"]))).all()


@pytest.mark.parametrize("name", [n for n in NAMES if MC.cases()[n]["o"]["margin"] == 0 and not np.isfinite(MC.cases()[n]["o"]["max_depth"]) and not np.isfinite(MC.cases()[n]["o"]["max_r2"])])
def test_agrees_with_predict_pixels(name):
    k = MC.cases()[name]; ref = MC.reference(name); pr = ref["proj"]
    X = k["X"]
    if k["align"] is not None:
        res = np.zeros(1, ALIGN_RESULT)[0]; res["c"], res["s"], res["t"] = k["align"]
        X, _ = localize.apply_alignment(res, X)
    with np.errstate(all="ignore"):
        px, ok = localize.predict_pixels(X, k["R_wc"], k["p_wc"], k["cam"])
    vis = pr["status"] == R.VISIBLE
    assert np.array_equal(ok, vis)
    assert R.adjacent_or_equal(px[vis, 0], pr["px"][vis].astype(np.float32)).all() and R.adjacent_or_equal(px[vis, 1], pr["py"][vis].astype(np.float32)).all()


def test_radius_closed_form():
    f, sig, z, ks, spx = 128.0, 0.05, 4.0, 2.5, 1.5
    o = R.options(k_sigma=ks, sigma_px=spx, r_min=0.5, r_max=500.0)
    pr = R.project([[0.0, 0.0, z]], sig * sig * np.eye(3)[None], MC.CAM_PLAIN, None, np.eye(3), np.zeros(3), None, o)
    assert pr["status"][0] == R.VISIBLE and (pr["px"][0], pr["py"][0]) == (320.0, 240.0)
    assert abs(pr["radius"][0] - ks * np.sqrt((f * sig / z) ** 2 + spx ** 2)) <= 1e-12
    # with neither covariance lambda is 0; a pose covariance alone widens it
    assert R.project([[0.0, 0.0, z]], None, MC.CAM_PLAIN, None, np.eye(3), np.zeros(3), None, o)["radius"][0] == ks * spx
    cc = np.diag([0.0, 0.0, 0.0, sig * sig, sig * sig, sig * sig])
    pr = R.project([[0.0, 0.0, z]], None, MC.CAM_PLAIN, None, np.eye(3), np.zeros(3), cc, o)
    assert abs(pr["radius"][0] - ks * np.sqrt((f * sig / z) ** 2 + spx ** 2)) <= 1e-12
    th = 0.01; cc = np.diag([th * th, 0.0, 0.0, 0.0, 0.0, 0.0])               # a rotation about the camera's x axis moves the axis point by f theta in y
    pr = R.project([[0.0, 0.0, z]], None, MC.CAM_PLAIN, None, np.eye(3), np.zeros(3), cc, o)
    assert abs(pr["radius"][0] - ks * np.sqrt((f * th) ** 2 + spx ** 2)) <= 1e-12


def test_view_limit_guards_the_radtan_fold_back():
    cam = dict(MC.CAM_RADTAN, distortion=(-0.3, 0.0, 0.0, 0.0))
    lim = localize.view_limit(cam)
    assert abs(lim - 1.0 / 0.9) < 1e-4                                         # d/dr (r (1 - 0.3 r^2)) = 0 at r^2 = 1 / 0.9, inside the image on every ray
    X = [[2.0 * 3.0, 0.0, 3.0], [0.3, 0.1, 3.0]]                               # r2 = 4: rad = -0.2, the point comes back at x_d = -0.4; and an ordinary point
    free = R.project(X, None, cam, None, np.eye(3), np.zeros(3), None, R.options())
    held = R.project(X, None, cam, None, np.eye(3), np.zeros(3), None, R.options(max_r2=lim))
    assert free["status"].tolist() == [R.VISIBLE, R.VISIBLE] and held["status"].tolist() == [R.OUTSIDE, R.VISIBLE]
    # a camera that never folds back inside r_max: the scan's end, squared
    assert localize.view_limit(MC.CAM_EQUI, r_max=5.0) == 25.0
    assert 1.5 < localize.view_limit(MC.CAM_RADTAN) < 2.5                      # the stock radtan camera: about the corners' r2 (1.76 .. 1.9)


def test_map_obs_applies_the_alignment_to_the_indexed_points():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(20, 3)); A = rng.normal(size=(20, 3, 3)); cov = A @ A.transpose(0, 2, 1)
    rec = np.zeros(6, MAP_MATCH)
    rec["index"] = [3, 7, 7, 19, 0, 11]; rec["m"]["status"] = [MATCH_OK, 2, MATCH_OK, MATCH_OK, 1, MATCH_OK]
    rec["m"]["und"] = rng.normal(size=(6, 2)).astype(np.float32)
    res = np.zeros(1, ALIGN_RESULT)[0]; res["c"], res["s"], res["t"] = MC.ALIGN
    obs, idx = localize.map_obs(rec, X, cov, res, 1.5, MC.CAM_RADTAN)
    assert idx.tolist() == [0, 2, 3, 5]
    p_w, cov_w = localize.apply_alignment(res, X, cov)
    k = rec["index"][idx]
    assert np.array_equal(obs["p_w"], p_w[k]) and np.array_equal(obs["cov_w"].reshape(-1, 3, 3), cov_w[k]) and np.array_equal(obs["uv"], rec["m"]["und"][idx].astype(np.float64))
    assert np.allclose(obs["sigma"], 1.5 / (0.5 * (458.654 + 457.296)))
    obs0, _ = localize.map_obs(rec, X, None, None, 1.5, MC.CAM_RADTAN)
    assert np.array_equal(obs0["p_w"], X[k]) and not obs0["cov_w"].any()
