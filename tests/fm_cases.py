"""The case table of the fundamental-matrix estimator's stage tests (CPU only): named, seeded point sets, each built to drive
fm_mask_block (larvio_amd/csrc/fe_track_dev.h) down one of its rarely taken paths, the oracle's answer for each (oracle/lvo.py), and a replay
of OpenCV's subset draws that says - from the generator alone, never from the kernel - which path a set reaches.
tests/test_fm_cases.py holds every case to its condition without a GPU; tests/test_gpu_fundamental_stages.py runs the table on the device."""
import functools
import numpy as np
from oracle import lvo

FILL = 0xA5
FM_THREADS, FM_WIDE_FROM, FM_MAX_N = 256, 512, 4096
FM_ROUND, FM_FIRST, FM_SECOND = 16, 2, 6
FM_WIN, FM_RNG_DRAWS = 256, 4096
FLT_EPSILON = float(np.finfo(np.float32).eps)

# ------------------------------------------------------------------------- cv::RNG and the subset draws
MWC_SEED = (1 << 64) - 1          # cv::RNG(-1): what every findFundamentalMat call starts from
MWC_A = 4164903690


def mwc_step(state):
    """one step of cv::RNG (multiply with carry) on Python integers: the new 64-bit state; the draw is its low 32 bits"""
    return ((state & 0xFFFFFFFF) * MWC_A + (state >> 32)) & ((1 << 64) - 1)


def collinear(pts):
    """haveCollinearPoints / d_have_collinear: the LAST point against every pair of the others, in double from float32 coordinates"""
    pts = np.asarray(pts, np.float32).astype(np.float64)
    i = len(pts) - 1
    for j in range(i):
        dx1, dy1 = pts[j, 0] - pts[i, 0], pts[j, 1] - pts[i, 1]
        for k in range(j):
            dx2, dy2 = pts[k, 0] - pts[i, 0], pts[k, 1] - pts[i, 1]
            if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def replay_draws(n, hyps, p1=None, p2=None, max_attempts=10000):
    """getSubset, `hyps` times in a row from a fresh generator, for a set of n points.  One record per hypothesis:
    dict(start = draws consumed before it, draws = [draws of each attempt], collinear = [did that attempt fail the collinearity test
    (in either image; always False without points)], idx = the seven indices it ends with, or None when all max_attempts attempts were collinear).
    The replay stops behind a hypothesis that fails, as the loop does."""
    state, used, out = MWC_SEED, 0, []
    for _ in range(hyps):
        rec = dict(start=used, draws=[], collinear=[], idx=None)
        for _ in range(max_attempts):
            idx, d = [], 0
            while len(idx) < 7:
                state = mwc_step(state); d += 1
                v = (state & 0xFFFFFFFF) % n
                if v not in idx:
                    idx.append(v)
            bad = p1 is not None and (collinear(p1[idx]) or collinear(p2[idx]))
            rec["draws"].append(d); rec["collinear"].append(bad); used += d
            if not bad:
                rec["idx"] = idx
                break
        out.append(rec)
        if rec["idx"] is None:
            break
    return out


def first_fallback(records):
    """Which event first takes the draw of these hypotheses (replay_draws records, in order) off the table-driven path, following the
    published schedule only: rounds of FM_FIRST, FM_SECOND, then FM_ROUND hypotheses, each round looking at the FM_WIN table draws behind
    its start.  -> (kind, round, hypothesis index) with kind 'table' (the window would pass the end of the FM_RNG_DRAWS-entry table),
    'window' (a subset of the round starts or ends behind the window) or 'collinear' (a first attempt fails the collinearity test); None when
    all the hypotheses are drawn from the table."""
    h, rnd = 0, 0
    while h < len(records):
        nr = FM_FIRST if rnd == 0 else FM_SECOND if rnd == 1 else FM_ROUND
        pos = records[h]["start"]
        if pos + FM_WIN > FM_RNG_DRAWS:
            return "table", rnd, h
        o = 0
        for r in range(nr):                                   # the kernel draws the whole round, also behind the hypothesis the loop stops at:
            if h + r >= len(records):                         # (records has to reach to the end of the round for an exact answer there)
                break
            d = records[h + r]["draws"][0]
            if o >= FM_WIN or o + d > FM_WIN:
                return "window", rnd, h + r
            o += d
        for r in range(nr):
            if h + r < len(records) and records[h + r]["collinear"][0]:
                return "collinear", rnd, h + r
        h += nr; rnd += 1
    return None


def round_up(iters):
    """hypotheses the round schedule has drawn by the time the loop stops after `iters` of them"""
    h, rnd = 0, 0
    while h < max(iters, 1):
        h += FM_FIRST if rnd == 0 else FM_SECOND if rnd == 1 else FM_ROUND; rnd += 1
    return h


# ------------------------------------------------------------------------- builders
K_CAM = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]])


def _project(X, R=None, t=None):
    X = X if R is None else (R @ X.T).T + t
    x = (K_CAM @ X.T).T
    return x[:, :2] / x[:, 2:]


def _yaw(th):
    return np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])


T_VIEW = np.array([0.2, 0.05, 0.03])


def two_view(n, outliers, seed, noise=0.3):
    """tests/test_gpu_frontend_stages.py::_two_view: a 0.05 rad yaw and a small translation, Gaussian pixel noise, the first
    int(outliers * n) correspondences moved by up to 40 px"""
    from tests.test_gpu_frontend_stages import _two_view
    return _two_view(n, outliers, seed, noise=noise)


def _f32(a, b):
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)


def _line_front(n, on_line, seed, outliers=0.0):
    """two-view set whose first `on_line` points of image 1 sit on the exact float row y = 100 (x as it was)"""
    p1, p2 = two_view(n, outliers, seed)
    p1 = p1.copy(); p1[:on_line, 1] = np.float32(100.0)
    return p1, p2


def _uniform(n, seed, scale=1.0):
    """both images uniform random: no geometry.  scale = 1e6 puts the coordinates where a 7-point model misses its OWN sample by more than
    0.05 px in double arithmetic, so no model ever counts more than 6 inliers"""
    rng = np.random.default_rng(seed)
    return _f32(rng.uniform(0, (752, 480), (n, 2)) * scale, rng.uniform(0, (752, 480), (n, 2)) * scale)


def _frozen(n, seed):
    p1, _ = two_view(n, 0.0, seed)
    return p1, p1.copy()


def _shift(n, seed):
    p1, _ = two_view(n, 0.0, seed)
    return p1, (p1 + np.array([3, 0], np.float32)).astype(np.float32)


def _rotation(n, seed):
    """p2 = the homography K R K^-1 of a 2 degree yaw applied to p1 (no translation: every F = [e]x H fits)"""
    p1, _ = two_view(n, 0.0, seed)
    H = K_CAM @ _yaw(np.deg2rad(2.0)) @ np.linalg.inv(K_CAM)
    q = np.column_stack([p1.astype(np.float64), np.ones(n)]) @ H.T
    return p1, (q[:, :2] / q[:, 2:]).astype(np.float32)


def _planar(n, seed, noise):
    rng = np.random.default_rng(seed)
    xy = rng.uniform([-3, -2], [3, 2], (n, 2))
    X = np.column_stack([xy, 6.0 + 0.3 * xy[:, 0] - 0.2 * xy[:, 1]])      # one slanted plane
    x1, x2 = _project(X), _project(X, _yaw(0.05), T_VIEW)
    return _f32(x1 + rng.normal(0, noise, x1.shape), x2 + rng.normal(0, noise, x2.shape))


def _repeated(seed):
    p1, p2 = two_view(10, 0.0, seed)
    return np.tile(p1, (3, 1)), np.tile(p2, (3, 1))


def _grid():
    """p1 = a 7 x 7 integer grid (60 px apart), p2 = the second view of the points of the plane z = 5 that project to it"""
    gx, gy = np.meshgrid(np.arange(7) * 60.0 + 100, np.arange(7) * 60.0 + 60)
    p1 = np.column_stack([gx.ravel(), gy.ravel()])
    rays = np.column_stack([p1, np.ones(49)]) @ np.linalg.inv(K_CAM).T
    X = rays * (5.0 + 0.4 * np.sin(np.arange(49)))[:, None]                # not one plane: depths vary
    return _f32(p1, _project(X, _yaw(0.05), T_VIEW))


@functools.lru_cache(maxsize=None)
def _cubic_set(want):
    """the first set of a seeded search on which the oracle's 7-point solver returns `want` models.  One and three models (the cubic's
    one-root and three-root branches) come from noisy two-view sets; none and two need an exact zero in the cubic (a0 == 0 or d == 0),
    which only sets of small integer coordinates give"""
    for k in range(3000):
        if want in (1, 3):
            p1, p2 = two_view(7, 0.0, 700 + k, noise=1.0)
        else:
            rng = np.random.default_rng(7000 + k)
            p1, p2 = _f32(rng.integers(0, 3, (7, 2)), rng.integers(0, 3, (7, 2)))
        if len(lvo.fundamental_7pt(p1, p2)) == want:
            return p1, p2
    raise AssertionError(f"no 7-point set with {want} models")


@functools.lru_cache(maxsize=None)
def _wide_set():
    return two_view(2000, 0.2, 41)


# ------------------------------------------------------------------------- the table
ALL = ("ransac", "mask", "F")
FIND = ("mask", "F")
# seeds and outlier shares below were tuned on the CPU against the oracle and are frozen; tests/test_fm_cases.py fails when one stops holding
OVERRUN_NARROW = dict(outliers=0.42, seed=2)       # 700 iterations (0.3 px noise against a 1 px threshold: 55 % already runs into the cap)
OVERRUN_WIDE = dict(outliers=0.42, seed=0)         # 730
CAP = dict(outliers=0.75, seed=0)
COLLINEAR_0 = dict(on_line=20, seed=4)             # hypothesis 1 draws three of the line's points; 777 iterations
COLLINEAR_LATE = dict(on_line=10, seed=0)          # hypothesis 14 (round 2) does; 108 iterations
# Window misfit.  The draws of a call depend on n alone (every call starts the generator afresh), so whether a round's subsets leave the
# 256-draw window is a property of n and of how far the loop runs, not of the seed or the noise:
#   n = 8   the first round that does not fit starts at hypothesis 120 (hypothesis 135 ends behind the window).  A two-view set of 8 points
#           stops after at most 9 hypotheses - a minimal sample's model always counts its own 7 points, and 7 of 8 makes the bound 9 -, so
#           no noise or seed gets there; misfit_n8 is kept as the small noisy set it is and stays on the table path.  misfit_n8_far gets there
#           the only way there is: coordinates so large (near 1e8) that no model counts even its own sample, so the loop runs to the cap.
#   n = 9, 10   every round fits until the table itself ends (hypotheses 328 / 360), and the bound is at most 24 / 54: unreachable; kept.
MISFIT = {8: dict(seed=0, outliers=0.25), 9: dict(seed=3, outliers=0.25), 10: dict(seed=3, outliers=0.4)}


def _table():
    T = {}

    def add(name, path, build, entries=ALL, thresh=1.0, conf=0.99, max_iters=1000, **expect):
        T[name] = dict(path=path, build=build, entries=entries, thresh=thresh, conf=conf, max_iters=max_iters, expect=expect)

    add("overrun_n60", "table overrun, 256 threads", lambda: two_view(60, **OVERRUN_NARROW), min_iters=600)
    add("overrun_n600", "table overrun, 512 threads", lambda: two_view(600, **OVERRUN_WIDE), min_iters=600)
    add("overrun_n500", "table overrun, 256 threads, two points a thread", lambda: two_view(500, 0.42, 3), min_iters=600)     # (745; the commit stage's wide case)
    add("cap_n40", "iteration cap", lambda: two_view(40, **CAP), iters=1000, ok=True)
    # uniform random pairs in the image: every model still fits the seven points it was made from, so the oracle's mask is NOT all zero (7 or 8
    # ones) - "no usable model" cannot happen there.  The same pairs a million times larger: no model counts more than 6, the mask is zero
    add("cap_sample_only_n30", "iteration cap, the best model fits little more than its own sample", lambda: _uniform(30, 5), thresh=0.05, iters=1000, ok=True, max_inliers=8)
    add("nothing_found_n30", "cap with no usable model", lambda: _uniform(30, 0, 1e6), thresh=0.05, iters=1000, ok=False)
    add("collinear_round0_n40", "collinear fallback in round 0", lambda: _line_front(40, **COLLINEAR_0), first_collinear=(0, 2))
    add("collinear_late_n40", "collinear fallback in a later round", lambda: _line_front(40, **COLLINEAR_LATE), first_collinear=(8, None))
    add("all_collinear_n20", "getSubset fails at once", lambda: _line_front(20, 20, 3), iters=0, ok=False, all_collinear=True)
    for n, kw in MISFIT.items():
        add(f"misfit_n{n}", "window misfit (not reached: see MISFIT)", lambda n=n, kw=kw: two_view(n, kw["outliers"], kw["seed"], noise=0.8), entries=("ransac",),
            misfit=False, min_iters_soft={8: 9, 9: 24, 10: 50}[n])
    add("misfit_n8_far", "window misfit", lambda: _uniform(8, 0, 1e6), entries=("ransac",), thresh=0.05, misfit=True, iters=1000, ok=False)
    for n in (15, 60):
        add(f"frozen_n{n}", "degenerate: frozen camera", lambda n=n: _frozen(n, 50 + n))
    add("shift_n60", "degenerate: constant shift", lambda: _shift(60, 52))
    add("rotation_n60", "degenerate: pure rotation", lambda: _rotation(60, 53))
    add("planar_n60", "degenerate: planar scene", lambda: _planar(60, 54, 0.0))
    add("planar_noisy_n60", "degenerate: planar scene, 0.3 px noise", lambda: _planar(60, 54, 0.3))
    add("repeated_n30", "degenerate: every correspondence three times", lambda: _repeated(55))
    add("grid_n49", "degenerate: integer grid", _grid)
    for want in (0, 1, 2, 3):
        add(f"cubic_{want}", f"7-point solver, {want} model(s)", lambda want=want: _cubic_set(want), entries=FIND, models=want)
    for n in (8, 11, 14):
        add(f"lmeds_exact_n{n}", "LMedS on exact data", lambda n=n: two_view(n, 0.0, 60 + n, noise=0.0))
    for n in (8, 14):
        add(f"lmeds_frozen_n{n}", "LMedS on a frozen camera", lambda n=n: _frozen(n, 70 + n))
    for mi in (0, 1, 2, 3, 7, 8, 9, 24, 25):
        add(f"max_iters_{mi}", "max_iters inside / at the edges of the first rounds", lambda: two_view(60, 0.3, 80), entries=("ransac",), max_iters=mi, max_iters_rule=True)
    for name, th, cf in (("thresh_0", 0.0, 0.99), ("thresh_neg", -1.0, 0.99), ("conf_0", 1.0, 0.0), ("conf_1", 1.0, 1.0)):
        add(f"default_{name}", "defaults", lambda: two_view(60, 0.3, 80), entries=FIND, thresh=th, conf=cf)
    for n in (511, 512, 513):
        add(f"width_n{n}", "workgroup width edge", lambda n=n: tuple(a[:n] for a in _wide_set()))
    add("capacity_n4096", "capacity", lambda: two_view(4096, 0.25, 90), ok=True)
    add("easy_n60", "fast path (10 % outliers)", lambda: two_view(60, 0.1, 91), ok=True)
    return T


CASES = _table()


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(name, path, p1, p2 (float32, contiguous, read-only), n, thresh, conf, max_iters, entries, expect)"""
    c = CASES[name]
    p1, p2 = _f32(*c["build"]())
    p1 = p1.copy(); p2 = p2.copy(); p1.setflags(write=False); p2.setflags(write=False)
    return dict(name=name, path=c["path"], p1=p1, p2=p2, n=len(p1), thresh=c["thresh"], conf=c["conf"], max_iters=c["max_iters"], entries=c["entries"], expect=c["expect"])


@functools.lru_cache(maxsize=None)
def oracle(name):
    """what the oracle says for the entries the case runs through:
    ransac = (ok, mask, iterations) of lvo.ransac_fundamental, find = (mask or None, F) of lvo.find_fundamental"""
    c = case(name)
    out = {}
    if "ransac" in c["entries"] or c["n"] >= 15:
        ok, mask, iters = lvo.ransac_fundamental(c["p1"], c["p2"], c["thresh"] if c["thresh"] > 0 else 3.0,
                                                 c["conf"] if 0 < c["conf"] < 1 else 0.99, c["max_iters"])
        out["ransac"] = (bool(ok), mask, iters)
    if "mask" in c["entries"] or "F" in c["entries"]:
        out["find"] = lvo.find_fundamental(c["p1"], c["p2"], c["thresh"], c["conf"])
    return out


@functools.lru_cache(maxsize=None)
def draws(name):
    """replay_draws of the case's set, to the end of the round in which the oracle's loop stops"""
    c = case(name)
    iters = oracle(name)["ransac"][2]
    return replay_draws(c["n"], round_up(iters), c["p1"], c["p2"])


def check_case(name):
    """the condition the case was built to meet, on the oracle and the replay alone"""
    c, e = case(name), case(name)["expect"]
    o = oracle(name)
    assert c["p1"].dtype == np.float32 and c["p1"].shape == c["p2"].shape == (c["n"], 2) and np.isfinite(c["p1"]).all() and np.isfinite(c["p2"]).all()
    assert c["n"] <= FM_MAX_N and ("ransac" not in c["entries"] or c["n"] >= 8)
    if "min_iters" in e:
        ok, _, iters = o["ransac"]
        assert ok and iters >= e["min_iters"], iters
        rec = draws(name)
        assert rec[iters - 1]["start"] + sum(rec[iters - 1]["draws"]) > FM_RNG_DRAWS and iters * 7 > FM_RNG_DRAWS
        assert first_fallback(rec)[0] == "table", first_fallback(rec)
    if "iters" in e:
        assert o["ransac"][2] == e["iters"], o["ransac"][2]
    if "ok" in e:
        assert o["ransac"][0] == e["ok"]
        if not e["ok"]:
            assert not o["ransac"][1].any()
            if "find" in o:
                assert o["find"][0] is not None and not o["find"][0].any() and not o["find"][1].any()
    if "first_collinear" in e:
        lo, hi = e["first_collinear"]
        iters = o["ransac"][2]
        rec = draws(name)
        first = next(i for i, r in enumerate(rec) if r["collinear"][0])
        assert lo <= first < (iters if hi is None else hi), (first, iters)
        assert first_fallback(rec) == ("collinear", 0 if first < 2 else 1 if first < 8 else 2 + (first - 8) // 16, first), first_fallback(rec)
    if e.get("all_collinear"):
        p = c["p1"]                                           # every triple of image 1 is collinear, so every attempt is: checked on all of them
        assert all(collinear(p[[i, j, k]]) for i in range(len(p)) for j in range(i) for k in range(j))
        rec = replay_draws(c["n"], 1, c["p1"], c["p2"], max_attempts=50)
        assert rec[0]["idx"] is None and all(rec[0]["collinear"])
    if "max_inliers" in e:
        assert 7 <= int(o["ransac"][1].sum()) <= e["max_inliers"]
    if "misfit" in e:
        ev = first_fallback(draws(name))
        if e["misfit"]:
            assert ev is not None and ev[0] == "window" and ev[2] < round_up(o["ransac"][2]), (ev, o["ransac"][2])
        else:                                                 # as far as a set of this size can go, and still on the table path
            assert o["ransac"][0] and o["ransac"][2] >= e["min_iters_soft"] and ev is None, (ev, o["ransac"][2])
    if "models" in e:
        assert len(lvo.fundamental_7pt(c["p1"], c["p2"])) == e["models"]
    if e.get("max_iters_rule"):
        free = lvo.ransac_fundamental(c["p1"], c["p2"], 1.0, 0.99, 1000)[2]
        assert free > 25 and o["ransac"][2] == min(max(c["max_iters"], 1), free), (o["ransac"][2], free)
    return o
