"""The named, seeded cases of the two-point alignment (lvk_align_ransac_2pt), shared by tests/test_align_ref.py (CPU) and
tests/test_gpu_align_stages.py / tests/test_gpu_align_frontend.py (GPU).  Sizes are where the kernels can go wrong - n = 2, 3, 63, 64, 65,
257, 1024 (the scoring sweeps 64 matches a step, the refinement 256), n_pairs = 1, 4, 5, 4096 (one wavefront, one workgroup, one
wavefront over, the cap) - not the workload's.

A case: dict(X (n, 3), uv (n, 2), pairs (P, 2) int32, R_wc, p_wc, opt (the non-default options; the noisy cases with many pairs use a threshold of two sigma, 0.004, so that
the best count is one model's alone - at five sigma every right pair holds every right match), planted: the degenerate conditions put
there on purpose (a subset of "tie", "pivot", "baseline"), want: what the restatement must find in it (status, flags), truth: (psi, t), good:
the matches that are right)."""
import numpy as np

from tests import align_ref as AR

MARGIN = 1e-6          # every margin of every case, apart from the planted degenerate ones


def rz(psi):
    c, s = np.cos(psi), np.sin(psi)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3); R[i, i] = c; R[j, j] = c; R[i, j] = -s; R[j, i] = s
    return R


LEVEL = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])      # camera z along world x, camera y down: d_z = -v exactly


def attitude(kind):
    if kind == "level":
        return LEVEL.copy()
    if kind == "yawed":
        return rz(2.1) @ LEVEL @ rot(0, -0.2) @ rot(2, 0.1)             # pitched 0.2 rad down, rolled 0.1
    if kind == "down":
        return rz(-0.8) @ LEVEL @ rot(0, -1.3)                          # looking steeply down
    raise ValueError(kind)


def scene(seed, n, outliers=0.0, noise=0.0, att="yawed", psi=0.7, t=(3.0, -2.0, 0.5), depth=(2.0, 8.0)):
    """n matches of a planted alignment: points in front of the camera, a share of them given another map position"""
    rng = np.random.default_rng([20261101, seed])
    R_wc = attitude(att); p_wc = np.array([1.5, 0.5, 1.2])
    uv = rng.uniform(-0.5, 0.5, (n, 2))
    z = rng.uniform(depth[0], depth[1], n)
    p_w = (np.concatenate([uv, np.ones((n, 1))], 1) * z[:, None]) @ R_wc.T + p_wc
    X = (p_w - np.asarray(t)) @ rz(psi)                              # rows: Rz^T (p_w - t)
    n_out = int(round(outliers * n))
    bad = rng.permutation(n)[:n_out]
    X[bad] = X[bad] + rng.uniform(-3.0, 3.0, (n_out, 3)) + np.sign(rng.normal(size=(n_out, 3))) * 0.5
    good = np.ones(n, bool); good[bad] = False
    uv = uv + noise * rng.normal(size=(n, 2))
    return dict(X=X, uv=uv, R_wc=R_wc, p_wc=p_wc, truth=(psi, np.asarray(t, np.float64)), good=good, opt={}, planted=set(), want={})


def _pairs(a):
    return np.asarray(a, np.int32).reshape(-1, 2)


def _random_pairs(seed, n, k):
    rng = np.random.default_rng([20261102, seed])
    i = rng.integers(0, n, k); j = rng.integers(0, n - 1, k); j += j >= i
    return _pairs(np.stack([i, j], 1))


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = {}
    # one pair, two matches: the smallest problem there is; the refinement has four equations for four unknowns
    k = scene(1, 2, noise=0.002); k["pairs"] = _pairs([(0, 1)]); k["opt"] = dict(min_inliers=2); k["planted"] = {"tie"}      # (both roots hold their own pair: a tie by construction)
    k["want"] = dict(status=AR.OK, hyp=0, root_w=0); C["n2_one_pair"] = k
    # five pairs, three of which name no pair at all: i == j, an index of -1, an index of n
    k = scene(2, 3, noise=0.002); k["pairs"] = _pairs([(0, 1), (1, 1), (-1, 2), (0, 3), (2, 0)]); k["opt"] = dict(min_inliers=3); k["planted"] = {"tie"}
    k["want"] = dict(status=AR.OK, reasons=[AR.R_INDEX]); C["n3_bad_indices_5"] = k
    # no noise, no outliers, every pair: every model holds all 63 matches - ties all the way, the first pair wins
    k = scene(33, 63); k["pairs"] = AR.draw_pairs(63); k["planted"] = {"tie"}; k["want"] = dict(status=AR.OK, hyp=0, n_inliers=63); C["n63_clean_all_pairs"] = k
    # four pairs (one workgroup exactly), 30 % wrong
    k = scene(44, 64, outliers=0.3, noise=0.002); k["pairs"] = _random_pairs(44, 64, 4); k["opt"] = dict(thresh=0.004); k["want"] = dict(status=AR.OK); C["n64_out30_4"] = k
    # 70 % wrong, every pair (2080)
    k = scene(50, 65, outliers=0.7, noise=0.002, att="down"); k["pairs"] = AR.draw_pairs(65); k["opt"] = dict(thresh=0.004)
    k["want"] = dict(status=AR.OK, reasons=[AR.R_DISC, AR.R_DEPTHS], flags=["two", "opposite"]); C["n65_out70_all_pairs"] = k
    # the cap of the pairs, drawn as the front-end draws them
    k = scene(63, 257, outliers=0.3, noise=0.002); k["pairs"] = AR.draw_pairs(257, 0, 11); k["opt"] = dict(thresh=0.004)
    k["want"] = dict(status=AR.OK, reasons=[AR.R_DISC], flags=["two"]); C["n257_out30_4096"] = k
    # both caps
    k = scene(72, 1024, outliers=0.7, noise=0.002, att="level"); k["pairs"] = AR.draw_pairs(1024, 0, 5); k["opt"] = dict(thresh=0.004); k["want"] = dict(status=AR.OK, reasons=[AR.R_DISC]); C["n1024_out70_4096"] = k
    # the cap of the matches with five pairs: one wavefront over a workgroup
    k = scene(8, 1024, outliers=0.3, noise=0.002); k["pairs"] = _random_pairs(8, 1024, 5); C["n1024_out30_5"] = k
    # a level camera: d_z = -v, and matches 0 and 2 have v = 0 exactly.  (0, 1), (1, 0): one bearing of the pair has d_z exactly 0 and the
    # other divides; (0, 2): both are 0, refused by min_dz
    k = scene(9, 12, noise=0.0, att="level"); k["uv"][0, 1] = 0.0; k["uv"][2, 1] = 0.0
    for q in (0, 2):                                                   # put the two points back on their new bearings
        z = 3.0 + q
        k["X"][q] = ((np.array([k["uv"][q, 0], 0.0, 1.0]) * z) @ k["R_wc"].T + k["p_wc"] - k["truth"][1]) @ rz(k["truth"][0])
    k["pairs"] = _pairs([(0, 1), (1, 0), (0, 2), (3, 4)]); k["planted"] = {"tie"}
    k["want"] = dict(status=AR.OK, reasons=[AR.R_MIN_DZ], flags=["dz_zero"], n_inliers=12); C["level_dz_zero_4"] = k
    # the planted tie: two pairs, both right, both with all eight matches - the lower index wins
    k = scene(10, 8); k["pairs"] = _pairs([(2, 5), (0, 1)]); k["planted"] = {"tie"}; k["want"] = dict(status=AR.OK, hyp=0, n_inliers=8); C["planted_tie"] = k
    # every match wrong: a model holds its own pair and little else
    k = scene(11, 64, outliers=1.0, noise=0.002); k["pairs"] = AR.draw_pairs(64); k["planted"] = {"tie"}; k["want"] = dict(status=AR.FEW_INLIERS); C["all_wrong"] = k
    # every map point on one vertical line: the xy baseline of every pair is 0
    k = scene(12, 16); k["X"][:, 0] = 1.25; k["X"][:, 1] = -0.5; k["pairs"] = AR.draw_pairs(16); k["planted"] = {"baseline"}
    k["want"] = dict(status=AR.NO_MODEL, reasons=[AR.R_BASELINE]); C["vertical_line"] = k
    # rank-deficient refinement: the pair (0, 1) lies nearer than min_depth, so its model does not count its own two matches; the
    # other ten matches are one map point and one observation, repeated - ten inliers, two independent rows
    k = scene(13, 12, depth=(0.4, 0.6)); k["opt"] = dict(min_depth=1.0)
    far = (np.array([0.1, -0.2, 1.0]) * 5.0) @ k["R_wc"].T + k["p_wc"]
    k["X"][2:] = (far - k["truth"][1]) @ rz(k["truth"][0]); k["uv"][2:] = (0.1, -0.2)
    k["pairs"] = _pairs([(0, 1)]); k["planted"] = {"pivot"}; k["want"] = dict(status=AR.SINGULAR, n_inliers=10); C["rank_deficient"] = k
    # too few to look at
    k = scene(14, 1); k["pairs"] = _pairs([(0, 0)]); k["want"] = dict(status=AR.NO_MODEL); C["n1"] = k
    k = scene(15, 5); k["pairs"] = _pairs([]); k["want"] = dict(status=AR.NO_MODEL); C["no_pairs"] = k
    for k in C.values():
        k["pairs"] = np.ascontiguousarray(k["pairs"], np.int32).reshape(-1, 2)
    _CASES = C
    return C


_REF = {}


def reference(name, kind="ld"):
    """the restatement's run of a case, computed once"""
    if (name, kind) not in _REF:
        k = cases()[name]
        _REF[name, kind] = AR.run(k["X"], k["uv"], k["pairs"], k["R_wc"], k["p_wc"], k["opt"], kind)
    return _REF[name, kind]


_BND = {}


def reference_bounds(name):
    if name not in _BND:
        k = cases()[name]
        _BND[name] = AR.bounds(k["X"], k["uv"], k["pairs"], k["R_wc"], k["p_wc"], reference(name), k["opt"])
    return _BND[name]


def exempt(name):
    """the margins a case's planted condition takes out of the 1e-6 rule"""
    planted = cases()[name]["planted"]
    return ({"pivot"} if "pivot" in planted else set())


def match_records(k, pad=0, fill=np.nan):
    """the ALIGN_MATCH array of a case, with `pad` records of `fill` behind it"""
    from larvio_amd._lib import ALIGN_MATCH
    n = len(k["X"])
    m = np.zeros(n + pad, ALIGN_MATCH)
    m["X"][:n] = k["X"]; m["u"][:n] = k["uv"][:, 0]; m["v"][:n] = k["uv"][:, 1]
    if pad:
        m["X"][n:] = fill; m["u"][n:] = fill; m["v"][n:] = fill
    return m


def pair_records(k, pad=0):
    from larvio_amd._lib import ALIGN_PAIR
    P = len(k["pairs"])
    p = np.zeros(P + pad, ALIGN_PAIR)
    p["i"][:P] = k["pairs"][:, 0]; p["j"][:P] = k["pairs"][:, 1]
    if pad:
        p["i"][P:] = 0x7FFFFFF0; p["j"][P:] = -7
    return p
