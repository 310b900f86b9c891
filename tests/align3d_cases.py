"""The named, seeded cases of the 3D-3D alignment (lvk_align_ransac_3d), shared by tests/test_align3d_ref.py (CPU) and
tests/test_gpu_align3d_stages.py (GPU), and the two synthetic sessions of the merge (tests/test_gpu_frontend_merge_map.py).  Sizes are where
the kernels can go wrong - n = 2, 63, 64, 65, 255, 256, 257, 1024 (the scoring sweeps 64 matches a step, the refinement 256), n_pairs = 1, 64,
4095, 4096 (one wavefront, sixteen workgroups, one under the cap, the cap) - not the workload's.

A case: dict(X, Y (n, 3), pairs (P, 2) int32, opt (the non-default options), want: what the restatement must find in it (status, hyp,
n_inliers, reasons), truth: (psi, t), good: the matches that are right, noise: the sigma below).  Good matches carry `noise` metres of Gaussian noise per
coordinate on Y; a wrong match has its Y somewhere else in the site."""
import numpy as np

from tests import align3d_ref as R3
from tests.align_cases import rz, _pairs, _random_pairs, pair_records      # noqa: F401  (pair_records is used by the GPU tests)

PSI, T = 0.7, (3.0, -2.0, 0.4)


def scene(seed, n, outliers=0.0, noise=0.0, psi=PSI, t=T):
    """n matches of a planted alignment over a site of 40 m x 40 m x 4 m, a share of them wrong"""
    rng = np.random.default_rng([20261201, seed])
    X = np.column_stack([rng.uniform(-20.0, 20.0, (n, 2)), rng.uniform(-2.0, 2.0, n)])
    Y = X @ rz(psi).T + np.asarray(t)
    Y = Y + noise * rng.normal(size=(n, 3))
    n_out = int(round(outliers * n))
    bad = rng.permutation(n)[:n_out]
    Y[bad] = np.column_stack([rng.uniform(-20.0, 20.0, (n_out, 2)), rng.uniform(-2.0, 2.0, n_out)])
    good = np.ones(n, bool); good[bad] = False
    return dict(X=X, Y=Y, truth=(psi, np.asarray(t, np.float64)), good=good, noise=float(noise), opt={}, want={})


_CASES = None


def cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    C = {}
    k = scene(1, 0); k["pairs"] = _pairs([]); k["want"] = dict(status=R3.NO_MODEL); C["n0"] = k
    k = scene(2, 1); k["pairs"] = _pairs([(0, 0)]); k["want"] = dict(status=R3.NO_MODEL); C["n1"] = k
    k = scene(3, 5, noise=0.01); k["pairs"] = _pairs([]); k["want"] = dict(status=R3.NO_MODEL); C["no_pairs"] = k
    # one pair, two matches: the smallest problem there is
    k = scene(4, 2, noise=0.01); k["X"][1] = k["X"][0] + (6.0, -3.0, 0.5); k["Y"][1] = k["Y"][0] + rz(PSI) @ (6.0, -3.0, 0.5) + (0.004, -0.003, 0.005)
    k["pairs"] = _pairs([(0, 1)]); k["opt"] = dict(min_inliers=2); k["want"] = dict(status=R3.OK, hyp=0, n_inliers=2); C["n2_one_pair"] = k
    # five pairs, three of which name no pair at all: i == j, an index of -1, an index of n
    k = scene(5, 3, noise=0.01); k["pairs"] = _pairs([(1, 1), (-1, 2), (0, 3), (0, 1), (2, 0)]); k["opt"] = dict(min_inliers=3)
    k["want"] = dict(status=R3.OK, hyp=3, reasons=[R3.R_INDEX]); C["n3_bad_indices_5"] = k
    # no noise, no outliers, every pair (1953): every model holds all 63 matches - ties all the way, the first pair wins
    k = scene(6, 63); k["pairs"] = R3.draw_pairs(63); k["want"] = dict(status=R3.OK, hyp=0, n_inliers=63, tie=True); C["n63_clean_all_pairs"] = k
    k = scene(7, 64, outliers=0.3, noise=0.01); k["pairs"] = _random_pairs(7, 64, 64); k["want"] = dict(status=R3.OK); C["n64_out30_64"] = k
    k = scene(8, 65, outliers=0.6, noise=0.01); k["pairs"] = R3.draw_pairs(65); k["want"] = dict(status=R3.OK, reasons=[R3.R_DZ, R3.R_LENGTH]); C["n65_out60_all_pairs"] = k
    # the 4096 boundary of the pair drawing: 91 matches have 4095 pairs, all of them taken; 92 have 4186, so 4096 are drawn
    k = scene(9, 91, outliers=0.3, noise=0.01); k["pairs"] = R3.draw_pairs(91, 0, 3); k["want"] = dict(status=R3.OK, n_pairs=4095); C["n91_out30_exhaustive_4095"] = k
    k = scene(10, 92, outliers=0.3, noise=0.01); k["pairs"] = R3.draw_pairs(92, 0, 3); k["want"] = dict(status=R3.OK, n_pairs=4096); C["n92_out30_drawn_4096"] = k
    k = scene(11, 255, outliers=0.8, noise=0.01); k["pairs"] = R3.draw_pairs(255, 0, 11); k["want"] = dict(status=R3.OK, n_pairs=4096); C["n255_out80_4096"] = k
    # one pair, and it is a right one
    k = scene(12, 256, outliers=0.3, noise=0.01); g = np.nonzero(k["good"])[0]; k["pairs"] = _pairs([(g[0], g[-1])]); k["want"] = dict(status=R3.OK, hyp=0); C["n256_out30_1"] = k
    k = scene(13, 257, outliers=0.6, noise=0.01); k["pairs"] = _random_pairs(13, 257, 64); k["want"] = dict(status=R3.OK); C["n257_out60_64"] = k
    # both caps
    k = scene(14, 1024, outliers=0.8, noise=0.01); k["pairs"] = R3.draw_pairs(1024, 0, 5); k["want"] = dict(status=R3.OK, n_pairs=4096); C["n1024_out80_4096"] = k
    # every solver rule refuses a pair of its own, the last pair is right.  Matches 0, 1: 14 cm apart; 2: its Y one metre too high;
    # 4: its Y one metre further from 5's than its X is
    k = scene(15, 12)
    k["X"][1] = k["X"][0] + (0.1, 0.1, 0.0); k["Y"][1] = k["Y"][0] + rz(PSI) @ (0.1, 0.1, 0.0)
    k["Y"][2, 2] += 1.0
    b = k["Y"][4, :2] - k["Y"][5, :2]; k["Y"][4, :2] += b / np.linalg.norm(b)
    k["pairs"] = _pairs([(0, 1), (2, 3), (4, 5), (6, 6), (7, 12), (8, 9)]); k["good"][[2, 4]] = False
    k["want"] = dict(status=R3.OK, hyp=5, n_inliers=10, reason_list=[R3.R_RHO, R3.R_DZ, R3.R_LENGTH, R3.R_INDEX, R3.R_INDEX, R3.R_MODEL]); C["refused_by_each_rule"] = k
    # the planted tie: two pairs, both right, both with all eight matches - the lower index wins
    k = scene(16, 8); k["pairs"] = _pairs([(2, 5), (0, 1)]); k["want"] = dict(status=R3.OK, hyp=0, n_inliers=8, tie=True); C["planted_tie"] = k
    # every match wrong; matches 0 and 1 agree with each other under another yaw, so their pair gives a model - it holds its own two
    k = scene(17, 64, outliers=1.0); k["Y"][1] = k["Y"][0] + rz(2.0) @ (k["X"][1] - k["X"][0]); k["pairs"] = R3.draw_pairs(64)
    k["want"] = dict(status=R3.FEW_INLIERS, hyp=0, n_inliers=2); C["all_wrong"] = k
    # the winner's inliers on one vertical line.  The pair (0, 1) straddles the line; its Y are 5/64 m off along x and in z, each the
    # other way: the lengths differ by 15.6 cm and so do the heights - inside the solver's 2 thresh - and the model is the truth (no yaw,
    # t = (3, -2, 0.5)), but it holds neither of its own two matches (d2 = 2 (5/64)^2 = 0.0122 > 0.1^2).  Every number is a short binary
    # fraction, so the model, the residuals (0) and all sums are exact in any arithmetic and any order.  The other eight matches share
    # (x, y) = (1.25, -0.5): every centred coordinate is 0, and so are D, C and W
    t = np.array([3.0, -2.0, 0.5])
    X = np.array([[2.25, -0.5, 0.0], [0.25, -0.5, 0.0]] + [[1.25, -0.5, 0.25 * q] for q in range(8)])
    Y = X + t; Y[0] += (0.078125, 0.0, 0.078125); Y[1] -= (0.078125, 0.0, 0.078125)
    k = dict(X=X, Y=Y, truth=(0.0, t), good=np.array([False, False] + [True] * 8), noise=0.0, opt={}, pairs=_pairs([(0, 1)]), want=dict(status=R3.SINGULAR, hyp=0, n_inliers=8))
    C["vertical_line"] = k
    for k in C.values():
        k["pairs"] = np.ascontiguousarray(k["pairs"], np.int32).reshape(-1, 2)
    _CASES = C
    return C


_REF, _BND, _FLG = {}, {}, {}


def reference(name, kind="ld"):
    """the restatement's run of a case, computed once"""
    if (name, kind) not in _REF:
        k = cases()[name]
        _REF[name, kind] = R3.run(k["X"], k["Y"], k["pairs"], k["opt"], kind)
    return _REF[name, kind]


def reference_bounds(name):
    if name not in _BND:
        k = cases()[name]
        _BND[name] = R3.bounds(k["X"], k["Y"], k["pairs"], reference(name), k["opt"])
    return _BND[name]


def flagged(name):
    """the deciding comparisons of a case that lie inside their V bound"""
    if name not in _FLG:
        k = cases()[name]
        _FLG[name] = R3.decisions(k["X"], k["Y"], k["pairs"], reference(name), k["opt"])
    return _FLG[name]


def match_records(k, pad=0, fill=np.nan):
    """the ALIGN3D_MATCH array of a case, with `pad` records of `fill` behind it"""
    from larvio_amd._lib import ALIGN3D_MATCH
    n = len(k["X"])
    m = np.zeros(n + pad, ALIGN3D_MATCH)
    m["X"][:n] = k["X"]; m["Y"][:n] = k["Y"]
    if pad:
        m["X"][n:] = fill; m["Y"][n:] = fill
    return m


# ------------------------------------------------------------------------------------------------ the two sessions of the merge
SESSIONS = dict(n_a=300, n_shared=120, n_new=80, psi=0.7, t=(3.0, -2.0, 0.4), sigma=0.01, r_dup=0.05)


def sessions(seed=20261202):
    """Session A: 300 points.  Session B: 120 of A's points seen again - in B's own frame (B -> A is yaw 0.7 rad, shift (3, -2, 0.4) m),
    with 1 cm of noise per coordinate and two descriptor bits inverted - plus 80 new points.  Covariances: (1 cm)^2 times a seeded
    factor between 1 and 4 on A, between 1 and 4 on B, so that neither side always wins a duplicate.
    -> dict(A: (X, cov, desc), B: (X, cov, desc), shared: A's indices seen again (B's first 120 rows, in that order), truth: (psi, t))"""
    S = SESSIONS
    rng = np.random.default_rng(seed)
    nA, nS, nN = S["n_a"], S["n_shared"], S["n_new"]
    XA = np.column_stack([rng.uniform(-20.0, 20.0, (nA, 2)), rng.uniform(-2.0, 2.0, nA)])
    dA = rng.integers(0, 256, (nA, 32), dtype=np.uint8)
    covA = (S["sigma"] ** 2 * rng.uniform(1.0, 4.0, nA))[:, None, None] * np.eye(3)
    shared = rng.permutation(nA)[:nS]
    t = np.asarray(S["t"], np.float64)
    YB = np.concatenate([XA[shared] + S["sigma"] * rng.normal(size=(nS, 3)), np.column_stack([rng.uniform(20.0, 40.0, (nN, 2)), rng.uniform(-2.0, 2.0, nN)])])
    XB = (YB - t) @ rz(S["psi"])                             # rows: Rz^T (Y - t)
    dB = np.concatenate([dA[shared].copy(), rng.integers(0, 256, (nN, 32), dtype=np.uint8)])
    for r in range(nS):
        for bit in rng.permutation(256)[:2]:
            dB[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    covB = (S["sigma"] ** 2 * rng.uniform(1.0, 4.0, nS + nN))[:, None, None] * np.eye(3)
    return dict(A=(XA, covA, dA), B=(XB, covB, dB), shared=shared, truth=(S["psi"], t))
