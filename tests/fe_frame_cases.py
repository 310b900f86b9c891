"""The case tables of the frame-stage tests and their builders (CPU only: images, points, the references of tests/fe_frame_ref.py and the
branch each case was built for).  tests/test_gpu_frame_stages.py runs every case on the GPU against the reference built here;
tests/test_fe_frame_ref.py runs the same builders without a GPU and holds each case to its branch assertions - one table, so the two
cannot drift apart."""
import functools
import numpy as np
from oracle import lvo
from tests import fe_frame_ref as R
from tests import fm_cases
from tests.test_gpu_frontend_edge import _texture, _crops
from tests.test_gpu_frontend_stages import _two_view

FILL = 0xA5
RADTAN = (0, None, (-0.05, 0.01, 0.0003, -0.0002))          # intrinsics follow the image size (cam_of)
FISHEYE = (1, None, (0.003, 0.0007, -0.002, 0.0002))


def cam_of(cam, w, h):
    return (cam[0], (0.6 * w, 0.6 * w, w / 2.0 - 0.5, h / 2.0 + 0.25), cam[2])


# =========================================================================== track stage
@functools.lru_cache(maxsize=None)
def frame_pair(w, h, pair):
    """(previous image, current image): 'shift' = crops of one texture 3 px / 2 px apart; 'unrelated' = another texture; 'half' = the shifted
    crop on the left half and the unrelated texture on the right (alive points and lost ones in one frame)"""
    tex = _texture(11, h + 120, w + 160)
    a, b = _crops(tex, w, h, [(40, 30), (43, 32)])
    if pair == "shift":
        return a, b
    other = _texture(12, h, w)
    if pair == "unrelated":
        return a, other
    c = b.copy(); c[:, w // 2:] = other[:, w // 2:]
    return a, c


@functools.lru_cache(maxsize=None)
def oracle_pyramid(w, h, pair, which, win, levels):
    p = lvo.LkPyramid(frame_pair(w, h, pair)[which], win, levels - 1)
    return p, p.orb_prepare()


def source_points(w, h, pair, count=120):
    p, _ = oracle_pyramid(w, h, pair, 0, 21, 1)
    g = p.good_features(count, 0.01, 12.0)
    border = np.array([[0.2, 0.4], [w - 1, h - 1], [w - 1.5, 0.5], [3.75, h / 2]], np.float32)
    return np.concatenate([g, border]).astype(np.float32)


def homography(kind, w, h):
    if kind == "I":
        return np.eye(3, dtype=np.float32)
    th = 0.012; c, s = np.cos(th), np.sin(th)                # a small in-plane rotation about the image centre plus a shift: starts near
    cx, cy = w / 2.0, h / 2.0                                # the right and bottom borders land outside the image
    return np.array([[c, -s, cx - c * cx + s * cy + 2.5], [s, c, cy - s * cx - c * cy + 1.5], [0, 0, 1]], np.float32)


def stored_descriptors(sc, fwd_ref):
    """Old tracks: the previous image's descriptors, except for a subset of the points the round trip keeps - there the oracle's CURRENT
    descriptor with exactly k bits inverted, k cycling through 57, 58, 59, 0, 100 and 256: distances on both sides of the gate"""
    w, h, pair, win, levels = sc["w"], sc["h"], sc["pair"], sc["win"], sc["levels"]
    _, planes0 = oracle_pyramid(w, h, pair, 0, win, levels)
    _, planes1 = oracle_pyramid(w, h, pair, 1, win, levels)
    stored, _ = lvo.orb_describe(planes0[0], planes0[1], sc["pts"])
    stored = stored.copy()
    cand = np.flatnonzero((fwd_ref["status"][:len(sc["pts"])] == R.ST_ALIVE) | (fwd_ref["status"][:len(sc["pts"])] == R.ST_ORB))
    rng = np.random.default_rng(5)
    flips = {}
    for j, i in enumerate(cand[::2]):
        k = (57, 58, 59, 0, 100, 256)[j % 6]
        dcur, _ = lvo.orb_describe(planes1[0], planes1[1], fwd_ref["curr"][i:i + 1])
        bits = np.unpackbits(dcur[0])
        bits[rng.permutation(256)[:k]] ^= 1
        stored[i] = np.packbits(bits)
        flips[int(i)] = k
    return stored, flips


# name: (w, h, variant, window, levels, is_new, H, pair, camera, all four status codes at least three times each)
TRACK_CASES = {
    "pipe_L4_old_I_half":     (320, 240, 2, 21, 4, 0, "I", "half", RADTAN, True),
    "pipe_L4_new_rot_half":   (320, 240, 2, 21, 4, 1, "rot", "half", RADTAN, False),
    "pipe_L3_old_rot_shift":  (336, 200, 2, 21, 3, 0, "rot", "shift", RADTAN, False),
    "pipe_L3_new_I_unrel":    (336, 200, 2, 21, 3, 1, "I", "unrelated", RADTAN, False),
    "pipe_L1_old_I_shift":    (320, 240, 2, 21, 1, 0, "I", "shift", RADTAN, False),
    "pipe_L2_new_rot_shift":  (320, 240, 2, 21, 2, 1, "rot", "shift", RADTAN, False),
    "pipe_L3_new_fisheye":    (320, 240, 2, 21, 3, 1, "I", "half", FISHEYE, False),
    "both21_L4_old_rot_half": (336, 200, 1, 21, 4, 0, "rot", "half", RADTAN, True),
    "both21_L2_new_I_half":   (320, 240, 1, 21, 2, 1, "I", "half", RADTAN, False),
    "both15_L4_old_I_half":   (320, 240, 1, 15, 4, 0, "I", "half", RADTAN, True),
    "both15_L1_new_rot_shift": (336, 200, 1, 15, 1, 1, "rot", "shift", RADTAN, False),
    "both31_L3_new_I_half":   (320, 240, 1, 31, 3, 1, "I", "half", RADTAN, False),
    "both31_L2_old_rot_unrel": (336, 200, 1, 31, 2, 0, "rot", "unrelated", RADTAN, False),
    "both21_L3_old_fisheye":  (320, 240, 1, 21, 3, 0, "I", "shift", FISHEYE, False),
    "pipe_L3_new_I_half_rev_edge":   (320, 240, 2, 21, 3, 1, "I", "half", RADTAN, False),
    "both21_L3_new_I_half_rev_edge": (320, 240, 1, 21, 3, 1, "I", "half", RADTAN, False),
}
# Source points whose round trip comes back between 1 px and 1.0001 px from where it started, found by bisection along x on the CPU oracle
# for exactly the configuration of the two *_rev_edge cases ('half' pair, 320 x 240, window 21, three levels, H = I): ST_REV by less than 1e-4 px
REV_EDGE_POINTS = np.array([[239.96250915527344, 82.04837799072266], [248.44839477539062, 87.58224487304688], [293.72552490234375, 112.00902557373047]], np.float32)


@functools.lru_cache(maxsize=None)
def track_case(name):
    """-> dict(w, h, variant, win, levels, is_new, H, cam, pair, pts, stored (or None), flips, ref)"""
    w, h, variant, win, levels, is_new, hk, pair, cam, all_codes = TRACK_CASES[name]
    sc = dict(w=w, h=h, variant=variant, win=win, levels=levels, is_new=is_new, H=homography(hk, w, h), cam=cam_of(cam, w, h), pair=pair,
              pts=source_points(w, h, pair), stored=None, flips={}, all_codes=all_codes, rev_edge=name.endswith("rev_edge"))
    if sc["rev_edge"]:
        sc["pts"] = np.concatenate([sc["pts"], REV_EDGE_POINTS])
    sc["ref"] = track_reference(sc, sc["pts"], 1, None)          # (old tracks: only to learn where the points go)
    if not is_new:
        sc["stored"], sc["flips"] = stored_descriptors(sc, sc["ref"])
        sc["ref"] = track_reference(sc, sc["pts"], 0, sc["stored"])
    return sc


def track_reference(sc, pts, is_new, stored, grid=None):
    p0, planes0 = oracle_pyramid(sc["w"], sc["h"], sc["pair"], 0, sc["win"], sc["levels"])
    p1, planes1 = oracle_pyramid(sc["w"], sc["h"], sc["pair"], 1, sc["win"], sc["levels"])
    return R.track_ref(p0, p1, planes0, planes1, pts, is_new, stored, sc["H"], sc["cam"], sc["w"], sc["h"], grid=grid, fill=FILL)


def check_track_case(sc):
    """what the case was built for, from the reference's output alone"""
    p0, _ = oracle_pyramid(sc["w"], sc["h"], sc["pair"], 0, sc["win"], sc["levels"])
    p1, _ = oracle_pyramid(sc["w"], sc["h"], sc["pair"], 1, sc["win"], sc["levels"])
    assert p0.n_levels == p1.n_levels == sc["levels"]
    st = sc["ref"]["status"]
    counts = [int((st == c).sum()) for c in range(4)]
    assert len(sc["pts"]) <= 130 and sum(counts) == len(st)
    assert counts[R.ST_ALIVE] >= 3 or sc["pair"] == "unrelated", counts
    if sc["all_codes"]:
        assert min(counts) >= 3, counts
    if sc["pair"] == "unrelated":
        assert counts[R.ST_FWD] + counts[R.ST_REV] > counts[R.ST_ALIVE], counts
    if not sc["is_new"]:                                      # the forced distances did what they were made for
        by_k = {k: [st[i] for i, kk in sc["flips"].items() if kk == k] for k in (57, 58, 59, 0, 100, 256)}
        assert by_k[57] and by_k[58] and by_k[59]
        assert all(s == R.ST_ALIVE for k in (0, 57, 58) for s in by_k[k]) and all(s == R.ST_ORB for k in (59, 100, 256) for s in by_k[k])
    if sc["rev_edge"]:                                        # the round trip itself, once more: just over the pixel
        pp = REV_EDGE_POINTS
        fwd, s0, _ = lvo.lk_track(p0, p1, pp, pp); back, s1, _ = lvo.lk_track(p1, p0, fwd, pp)
        dis = np.hypot((back - pp)[:, 0].astype(np.float64), (back - pp)[:, 1].astype(np.float64)).astype(np.float32)
        assert s0.all() and s1.all() and ((dis > 1) & (dis < np.float32(1.0001))).all(), dis
        assert (st[-len(pp):] == R.ST_REV).all()
    assert sc["ref"]["point_levels"] == (len(st) + int((st != R.ST_FWD).sum())) * sc["levels"]
    return counts


# =========================================================================== commit stage
def _status_pattern(pattern, n, nt, rng):
    st = np.full(n, R.ST_FWD, np.uint8)
    other = rng.integers(1, 4, n).astype(np.uint8)            # what the points that are not alive carry: all three losing codes
    if pattern == "all":
        st[:] = R.ST_ALIVE; return st, n
    if pattern == "none":
        return other, 0
    if pattern == "third":
        st = other; st[::3] = R.ST_ALIVE; return st, (n + 2) // 3
    if pattern == "lane63":
        st = other; st[63::64] = R.ST_ALIVE; return st, n // 64
    if pattern == "last_chunk":
        st = other; first = nt * ((n - 1) // nt) if n else 0
        st[first:] = R.ST_ALIVE; return st, n - first
    if pattern == "random4":
        st = rng.integers(0, 4, n).astype(np.uint8); return st, int((st == 0).sum())
    kind, a, o, r = pattern                                   # ("counts", alive, orb, rev): exact counts, the rest lost forward, shuffled
    assert kind == "counts" and a + o + r <= n
    st[:a] = R.ST_ALIVE; st[a:a + o] = R.ST_ORB; st[a + o:a + o + r] = R.ST_REV
    return rng.permutation(st), a


def _nt(cap):
    return R.FM_THREADS_WIDE if cap > R.FM_WIDE_FROM else R.FM_THREADS


# name: dict(mode, cap, n, pattern, seed, outliers, noise, dst_n (before), expect = the branch record's fields this case was built for)
def _commit_table():
    T = {}
    def add(name, mode, cap, n, pattern, expect, dst_n=0, outliers=0.2, noise=0.3, seed=None, dst_n_from_kept=None, und_from=None):
        T[name] = dict(mode=mode, cap=cap, n=n, pattern=pattern, expect=expect, dst_n=dst_n, outliers=outliers, noise=noise,
                       seed=len(T) + 100 if seed is None else seed, dst_n_from_kept=dst_n_from_kept, und_from=und_from)
    # compaction across chunk and wavefront edges, both widths.  With 256 threads no cap reaches 2 NT + 1 points (the width changes at cap > 512):
    # n = 2 NT = cap = 512 is the largest set, two whole chunks
    sizes = {64: (0, 1, 63, 64), 512: (65, 255, 256, 257, 512), 513: (0, 1, 64, 65, 511, 512, 513), 2048: (63, 513, 1025, 2048)}
    patterns = ("all", "none", "third", "lane63", "last_chunk", "random4")
    k = 0
    for cap, ns in sizes.items():
        for n in ns:
            for j in range(3 if n > 1 else 1):                # three of the six patterns per size, rotating: every pattern meets every edge kind
                pat = patterns[(k + 2 * j) % 6] if n > 1 else "all"
                add(f"m0_cap{cap}_n{n}_{pat}", 0, cap, n, pat, dict(width=_nt(cap), fail=(), clipped=False))
            k += 1
    for cap in (512, 2048):                                   # the patterns the rotation did not give the largest sets
        for pat in ("lane63", "last_chunk", "third"):
            add(f"m0_cap{cap}_n{cap}_{pat}_full", 0, cap, cap, pat, dict(width=_nt(cap), fail=(), clipped=False))
    add("m0_cap2048_n1025_last_chunk_2nt1", 0, 2048, 1025, "last_chunk", dict(width=512, m=1, method="none", fail=()))
    # the mask dispatch inside the commit
    for m in (0, 6, 7, 8, 14, 15, 16):
        add(f"m0_dispatch_m{m}", 0, 64, 40, ("counts", m, 5, 5), dict(width=256, m=m, method=None if m == 0 else R.mask_method(m), fail=()))
    for m in (8, 15):                                         # 512 threads, a dozen points: the hypothesis machinery runs on the first 256
        add(f"m0_dispatch_wide_m{m}", 0, 513, 22, ("counts", m, 3, 3), dict(width=512, m=m, method=R.mask_method(m), fail=()))
    # mode 1: the threshold, the append, the clipping (noise-free inliers only: the mask keeps them all, so `kept` is known)
    add("m1_m19_fails", 1, 64, 30, ("counts", 19, 4, 4), dict(m=19, method=None, fail=("m",), clipped=False), dst_n=7)
    add("m1_m20_appends", 1, 64, 30, ("counts", 20, 4, 4), dict(m=20, method="ransac", fail=(), clipped=False), dst_n=7)
    add("m1_wide_appends", 1, 513, 300, "third", dict(width=512, m=100, method="ransac", fail=(), clipped=False), dst_n=101)
    add("m1_clip_by_1", 1, 64, 40, ("counts", 25, 5, 5), dict(m=25, kept=25, fail=(), clipped=True), outliers=0, noise=0, dst_n_from_kept=1)
    add("m1_clip_by_many", 1, 64, 64, "all", dict(m=64, kept=64, fail=(), clipped=True), outliers=0, noise=0, dst_n=50)
    add("m1_clip_full_set", 1, 64, 30, ("counts", 22, 4, 4), dict(m=22, kept=22, fail=(), clipped=True), outliers=0, noise=0, dst_n=64)
    add("m1_clip_wide_by_1", 1, 513, 100, ("counts", 60, 20, 20), dict(width=512, m=60, kept=60, fail=(), clipped=True), outliers=0, noise=0, dst_n_from_kept=1)
    add("m1_exactly_full", 1, 64, 40, ("counts", 25, 5, 5), dict(m=25, kept=25, fail=(), clipped=False), outliers=0, noise=0, dst_n_from_kept=0)
    # mode 2: cnt[0] >= cnt[1] >= m always, so a count at 19 takes the ones behind it below 20 with it; each is also shown at 20
    add("m2_cnt0_19", 2, 64, 29, ("counts", 15, 2, 2), dict(fail=("cnt0", "cnt1", "m"), method=None), outliers=0, noise=0)
    add("m2_cnt0_20", 2, 64, 30, ("counts", 20, 0, 0), dict(fail=(), m=20, kept=20), outliers=0, noise=0)
    add("m2_cnt1_19", 2, 64, 30, ("counts", 17, 2, 6), dict(fail=("cnt1", "m"), method=None), outliers=0, noise=0)
    add("m2_cnt1_20", 2, 64, 30, ("counts", 20, 0, 5), dict(fail=(), m=20, kept=20), outliers=0, noise=0)
    add("m2_m19", 2, 64, 30, ("counts", 19, 5, 3), dict(fail=("m",), m=19, method=None), outliers=0, noise=0)
    add("m2_m20", 2, 64, 31, ("counts", 20, 5, 3), dict(fail=(), m=20, kept=20), outliers=0, noise=0)
    add("m2_mask_leaves_fewer_than_20", 2, 64, 30, ("counts", 24, 3, 3), dict(fail=("kept",), m=24, method="ransac"), outliers=1 / 3, noise=0.1, seed=7)
    add("m2_wide", 2, 2048, 700, "third", dict(width=512, fail=(), m=234, method="ransac"))
    # the estimator off its fast path inside the commit: the alive points are a set of tests/fm_cases.py, in its order (und_from), so the
    # path that set was proved to reach is the path this launch takes.  Table overrun at both widths, a frozen camera, and a set whose
    # every subset is collinear (no model: the mask drops every point)
    add("m0_fm_overrun", 0, 64, 64, ("counts", 60, 2, 2), dict(width=256, m=60, method="ransac", fail=()), und_from="overrun_n60")
    add("m0_fm_overrun_wide", 0, 513, 513, ("counts", 500, 6, 7), dict(width=512, m=500, method="ransac", fail=()), und_from="overrun_n500")
    add("m0_fm_frozen", 0, 64, 64, ("counts", 60, 2, 2), dict(width=256, m=60, kept=60, method="ransac", fail=()), und_from="frozen_n60")
    add("m0_fm_all_collinear", 0, 64, 30, ("counts", 20, 5, 5), dict(width=256, m=20, kept=0, method="ransac", fail=()), und_from="all_collinear_n20")
    return T


COMMIT_CASES = _commit_table()


@functools.lru_cache(maxsize=None)
def commit_case(name):
    """-> dict(mode, cap, src, dst, state, ref_dst, ref_state, branch, expect, expect_m)"""
    c = COMMIT_CASES[name]
    mode, cap, n = c["mode"], c["cap"], c["n"]
    rng = np.random.default_rng(c["seed"])
    status, expect_m = _status_pattern(c["pattern"], n, _nt(cap), rng)
    src = dict(pts=rng.uniform(0, 300, (n, 2)).astype(np.float32), curr=rng.uniform(0, 300, (n, 2)).astype(np.float32), status=status,
               und=np.zeros((n, 2, 2), np.float32), desc=rng.integers(0, 256, (n, 32)).astype(np.uint8),
               id=rng.integers(0, 2 ** 40, n).astype(np.uint64), init=rng.uniform(-1, 300, (n, 2)).astype(np.float32), life=rng.integers(1, 5000, n).astype(np.int32))
    # the alive points see one two-view scene (with its share of gross outliers, in order); the others carry pairs nothing may read as inliers
    alive = np.flatnonzero(status == R.ST_ALIVE)
    src["und"][:, 0] = rng.uniform(0, 700, (n, 2)); src["und"][:, 1] = rng.uniform(0, 700, (n, 2))
    if c["und_from"]:
        fm = fm_cases.case(c["und_from"])
        assert len(alive) == fm["n"]
        src["und"][alive, 0] = fm["p1"]; src["und"][alive, 1] = fm["p2"]
    elif len(alive):
        x1, x2 = _two_view(len(alive), c["outliers"], c["seed"], noise=c["noise"])
        perm = rng.permutation(len(alive))                    # outliers anywhere in the order, not in front
        src["und"][alive, 0] = x1[perm]; src["und"][alive, 1] = x2[perm]
    if mode != 0:
        src["id"] = src["init"] = src["life"] = None
    dst = {k: R.filled(s, t, FILL) for k, (s, t) in dict(id=(cap, np.uint64), pts=((cap, 2), np.float32), ppts=((cap, 2), np.float32),
                                                         init=((cap, 2), np.float32), life=(cap, np.int32), desc=((cap, 32), np.uint8)).items()}
    state = dict(next_id=1000 + c["seed"], dst_n=c["dst_n"], n_new=n if mode else 17, boot_ok=-7)
    if c["dst_n_from_kept"] is not None:                      # append so that dst_n + kept = cap + this
        _, _, br = R.commit_ref(mode, cap, src, dst, state)
        state["dst_n"] = cap + c["dst_n_from_kept"] - br["kept"]
    if mode == 1:                                             # what the set held before the append
        d = state["dst_n"]
        dst["id"][:d] = np.arange(d) + 5; dst["life"][:d] = 9; dst["pts"][:d] = rng.uniform(0, 300, (d, 2)); dst["ppts"][:d] = rng.uniform(0, 300, (d, 2))
        dst["init"][:d] = -1; dst["desc"][:d] = rng.integers(0, 256, (d, 32))
    ref_dst, ref_state, br = R.commit_ref(mode, cap, src, dst, state)
    return dict(mode=mode, cap=cap, n=n, src=src, dst=dst, state=state, ref_dst=ref_dst, ref_state=ref_state, branch=br, expect=c["expect"], expect_m=expect_m,
                pattern=c["pattern"], und_from=c["und_from"])


def check_commit_case(cc):
    """the branch the case was built for, from the reference's record"""
    br, c = cc["branch"], cc
    assert br["width"] == _nt(c["cap"])
    assert br["m"] == c["expect_m"], (br["m"], c["expect_m"])
    for k, v in c["expect"].items():
        assert br[k] == v, (k, br[k], v)
    if c["pattern"] == "random4":
        assert c["n"] < 4 or len(set(c["src"]["status"].tolist())) == 4
    if "method" not in c["expect"] and not br["fail"]:
        assert br["method"] == (None if br["m"] == 0 else R.mask_method(br["m"]))
    if c["und_from"]:                                         # the estimator sees exactly that set: its path (tests/test_fm_cases.py) and its mask
        fm_cases.check_case(c["und_from"])
        assert br["kept"] == int(fm_cases.oracle(c["und_from"])["find"][0].sum())
    s0, s1 = c["state"], c["ref_state"]
    if c["mode"] == 1:
        if br["fail"]:
            assert s1 == s0 and all(np.array_equal(c["dst"][k], c["ref_dst"][k]) for k in c["dst"])
        else:
            assert s1["next_id"] == s0["next_id"] + br["kept"] and s1["n_new"] == 0 and s1["dst_n"] == min(s0["dst_n"] + br["kept"], c["cap"])
            assert br["clipped"] == (s0["dst_n"] + br["kept"] > c["cap"])
            assert all(np.array_equal(c["dst"][k][:s0["dst_n"]], c["ref_dst"][k][:s0["dst_n"]]) for k in c["dst"])
    if c["mode"] == 2:
        assert s1["boot_ok"] == (0 if br["fail"] else 1) and s1["dst_n"] == (0 if br["fail"] else br["kept"])
        if not br["fail"]:
            assert (c["ref_dst"]["init"][:br["kept"]] == -1).all() and (c["ref_dst"]["life"][:br["kept"]] == 2).all() and s1["n_new"] == 0
        if br["fail"] == ("kept",):
            assert 0 < br["kept"] < 20 and br["scratch"] == br["kept"]
    if c["mode"] == 0:
        assert s1["dst_n"] == br["kept"] and s1["next_id"] == s0["next_id"] and s1["n_new"] == s0["n_new"] and s1["boot_ok"] == s0["boot_ok"]


# =========================================================================== message stage
# name: (n, cap, prev_is_last, camera)
MSG_CASES = {f"n{n}_last{pl}_{'fisheye' if cam is FISHEYE else 'radtan'}": (n, cap, pl, cam)
             for n, cap in ((0, 5), (1, 1), (63, 64), (64, 64), (65, 130), (257, 300)) for pl in (0, 1) for cam in (RADTAN, FISHEYE)
             if cam is RADTAN or n in (65, 257)}
MSG_DT = (0.05, 0.125)
MSG_STATE = dict(n_msg=-3, n_host=-4, msg_features=1000, msg_count=41)


@functools.lru_cache(maxsize=None)
def msg_case(name):
    n, cap, prev_is_last, cam = MSG_CASES[name]
    rng = np.random.default_rng(n + 7 * prev_is_last)
    w, h = 320, 240
    ts = dict(id=rng.integers(0, 2 ** 50, cap).astype(np.uint64), pts=rng.uniform(0, (w - 1, h - 1), (cap, 2)).astype(np.float32),
              ppts=rng.uniform(0, (w - 1, h - 1), (cap, 2)).astype(np.float32), init=rng.uniform(0, (w - 1, h - 1), (cap, 2)).astype(np.float32))
    ts["init"][::3] = -1                                      # the sentinel on every third track ...
    if n > 4:
        ts["init"][1] = (-1, 77.5); ts["init"][2] = (12.25, -1); ts["init"][4] = (-1, -1)     # ... and two real points that only look like it
    cam = cam_of(cam, w, h)
    out, init, state = R.msg_ref(ts, cap, n, cam, MSG_DT[0], MSG_DT[1], prev_is_last, MSG_STATE, fill=FILL)
    return dict(n=n, cap=cap, prev_is_last=prev_is_last, cam=cam, set=ts, ref_out=out, ref_init=init, ref_state=state)


def check_msg_case(mc):
    n, init0, init1 = mc["n"], mc["set"]["init"], mc["ref_init"]
    real = ~((init0[:n, 0] == -1) & (init0[:n, 1] == -1))
    assert (init1[:n] == -1).all() and np.array_equal(init1[n:].view(np.uint32), init0[n:].view(np.uint32))
    assert np.array_equal(mc["ref_out"]["u_init"][:n] != -1, real) or n == 0
    if n > 4:
        assert real[1] and real[2] and not real[4] and not real[0]
        assert (mc["ref_out"]["u_init_vel"][:n][~real] == 0).all() and (mc["ref_out"]["u_init_vel"][:n][real] != 0).all()
    assert mc["ref_state"] == dict(n_msg=n, n_host=n, msg_features=1000 + n, msg_count=42)
    assert (mc["ref_out"][n:].view(np.uint8) == FILL).all()
