"""Named cases of the map build (lvk_map_build), generated from fixed seeds.  case(name) -> dict(X, cov, desc, score, opt, want):
the inputs (cov / desc / score may be None), the options as keywords of ops.map_build_options, and `want`, the case's planted property:

    dup / bad / uncertain / out_of_range   the exact set of indices with that status
    order                                   the exact d_order

reference(name) is the judge's answer (tests/map_build_ref.build), computed once and shared by the tests."""
import functools

import numpy as np

from tests import map_build_ref as R

NAN, INF = float("nan"), float("inf")


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip(d, bits):
    """a copy of descriptor d with the given bit positions (0..255) inverted"""
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _cov(rng, n, scale=1e-3):
    A = rng.normal(0.0, 1.0, (n, 3, 3))
    return scale * (A @ A.transpose(0, 2, 1)) + 1e-6 * np.eye(3)


def _from_bits(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def generic(n, seed, r_dup=0.25, spread=4.0, score="cov", with_cov=True, max_score=0.0):
    """n points: three quarters are random, a quarter are near copies of earlier ones (moved by less than r_dup / 4, one descriptor bit
    inverted), shuffled; one NaN coordinate from n = 8 on.  A few points per occupied cell at the default spread from a few thousand points on."""
    rng = np.random.default_rng(seed)
    m = n - n // 4
    X = rng.uniform(-spread, spread, (m, 3)); d = _desc(rng, m)
    src = rng.integers(0, max(m, 1), n // 4)
    Xc = X[src] + rng.uniform(-1.0, 1.0, (n // 4, 3)) * (r_dup / 8.0)
    dc = np.array([flip(d[s], [int(rng.integers(0, 256))]) for s in src], np.uint8).reshape(-1, 32)
    X = np.concatenate([X, Xc]); d = np.concatenate([d, dc])
    p = rng.permutation(n)
    X, d = X[p], d[p]
    if n >= 8:
        X[int(rng.integers(0, n)), 1] = NAN
    cov = _cov(rng, n) if with_cov else None
    sc = None if score == "cov" else rng.uniform(0.0, 1.0, n)
    return dict(X=X, cov=cov, desc=d, score=sc, opt=dict(r_dup=r_dup, max_score=max_score), want={})


def _scores_only(scores, seed=1):
    """points far apart, no de-duplication: the order is the scores' alone"""
    rng = np.random.default_rng(seed)
    n = len(scores)
    return dict(X=rng.uniform(-50.0, 50.0, (n, 3)), cov=None, desc=_desc(rng, n), score=np.asarray(scores, np.float64), opt={}, want={})


def _pairs(points, r_dup, **opt):
    """points: a list of (X, descriptor, score); filler points far away are appended so that more than one cell is occupied"""
    rng = np.random.default_rng(99)
    X = np.array([p[0] for p in points], np.float64); d = np.array([p[1] for p in points], np.uint8); s = np.array([p[2] for p in points], np.float64)
    fx = rng.uniform(100.0, 200.0, (5, 3)); fd = _desc(rng, 5)
    return dict(X=np.concatenate([X, fx]), cov=None, desc=np.concatenate([d, fd]), score=np.concatenate([s, np.full(5, 9.0)]), opt=dict(r_dup=r_dup, **opt), want={})


def _bad_variants(score_given):
    rng = np.random.default_rng(7)
    n = 48
    X = rng.uniform(-3.0, 3.0, (n, 3)); cov = _cov(rng, n); d = _desc(rng, n); s = rng.uniform(0.1, 1.0, n)
    X[3, 0] = NAN; X[5, 2] = INF; X[6, 1] = -INF
    cov[8, 0, 1] = NAN; cov[9, 2, 2] = INF; cov[10, 1, 1] = -1e-300; cov[11, 2, 0] = -INF
    cov[12, 0, 0] = -0.0                                                 # not negative: stays
    bad = {3, 5, 6, 8, 9, 10, 11}
    if score_given:
        s[14] = NAN; s[15] = INF; s[16] = -1e-320; s[17] = -0.0          # -0 is not < 0: stays, and sorts with the zeros
        cov[18] = np.diag([1e308, 1e308, 1e308])                         # its trace overflows, but the score is given: stays
        bad |= {14, 15, 16}
    else:
        cov[18] = np.diag([1e308, 1e308, 1e308])                         # finite entries, a trace that is not: BAD
        bad |= {18}
    return dict(X=X, cov=cov, desc=d, score=s if score_given else None, opt=dict(r_dup=0.01), want=dict(bad=sorted(bad), dup=[]))


def _crowd(m, seed):
    """m mutual duplicates in one cell among 40 scattered points: only the best of the crowd stays"""
    rng = np.random.default_rng(seed)
    base = _desc(rng, 1)[0]
    Xc = np.array([0.3, 0.3, 0.3]) + rng.uniform(-0.01, 0.01, (m, 3))
    dc = np.array([flip(base, rng.integers(0, 256, 3).tolist()) for _ in range(m)], np.uint8)
    sc = rng.permutation(m).astype(np.float64) + 1.0
    Xf = rng.uniform(5.0, 50.0, (40, 3)); df = _desc(rng, 40); sf = rng.uniform(0.0, 1.0, 40)
    X = np.concatenate([Xf[:20], Xc, Xf[20:]]); d = np.concatenate([df[:20], dc, df[20:]]); s = np.concatenate([sf[:20], sc, sf[20:]])
    best = 20 + int(np.argmin(sc))
    return dict(X=X, cov=None, desc=d, score=s, opt=dict(r_dup=1.0), want=dict(dup=[i for i in range(20, 20 + m) if i != best]))


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("n") and name[1:].split("_")[0].isdigit():
        n = int(name[1:].split("_")[0])
        if name.endswith("_score_nocov"):
            return generic(n, 11 + n, score="given", with_cov=False)
        if name.endswith("_nodedup"):
            return generic(n, 11 + n, r_dup=0.0)
        return generic(n, 11 + n, max_score=0.009 if n >= 255 else 0.0)
    if name == "equal_scores":
        return _scores_only(np.full(700, 1.5))
    if name == "low_byte_scores":
        return _scores_only(_from_bits(np.float64(1.0).view(np.uint64) + rng.integers(0, 256, 600).astype(np.uint64)))
    if name == "high_byte_scores":                                       # only bits 56..62 differ
        return _scores_only(_from_bits((rng.integers(0, 0x80, 500).astype(np.uint64) << np.uint64(56)) | np.uint64(0x000F000000000001)))
    if name == "every_byte_scores":
        b = rng.integers(0, 256, (1000, 8)).astype(np.uint8); b[:, 7] &= 0x7F
        v = b.view(np.uint64).reshape(-1)
        v[v >= np.uint64(0x7FF0000000000000)] = np.uint64(0x3FF0000000000000)
        return _scores_only(_from_bits(v))
    if name == "one_byte_each_scores":                                   # byte k of score k % 8 is the only one that differs from its neighbours
        v = np.array([(int(rng.integers(1, 0x7F if k % 8 == 7 else 256)) << (8 * (k % 8))) for k in range(320)], np.uint64)
        return _scores_only(_from_bits(v))
    if name == "denormal_scores":
        return _scores_only(_from_bits(rng.integers(0, 1 << 20, 300).astype(np.uint64)))
    if name == "signed_zero_scores":
        s = rng.choice(np.array([0.0, -0.0, 5e-324, 1e-310]), 200)
        k = _scores_only(s)
        zeros = [i for i in range(200) if s[i] == 0.0]
        k["want"] = dict(order_head=zeros)                               # every zero, of either sign, in index order, ahead of the rest
        return k
    if name == "score_from_cov":
        k = generic(400, 5); k["want"] = {}
        return k
    if name == "score_given_with_cov":
        return generic(400, 5, score="given")
    if name == "no_cov_no_score":
        k = generic(300, 6, with_cov=False)
        return k
    if name == "bad_variants_score":
        return _bad_variants(True)
    if name == "bad_variants_trace":
        return _bad_variants(False)
    if name == "max_score_edge":
        s = rng.uniform(0.0, 1.0, 100); m = 0.625
        s[10] = m; s[11] = np.nextafter(m, 2.0); s[12] = np.nextafter(m, 0.0); s[13] = m; s[14] = np.nextafter(m, 2.0)
        k = _scores_only(s); k["opt"] = dict(max_score=m)
        k["want"] = dict(uncertain=sorted(int(i) for i in np.nonzero(s > m)[0]))
        assert 11 in k["want"]["uncertain"] and 10 not in k["want"]["uncertain"]
        return k
    if name == "cell_range_edge":                                        # r_dup = 1: the cell is floor(X)
        d = _desc(rng, 1)[0]
        hi = float(2 ** 20 - 1)
        pts = [((hi + 0.5, 0.5, 0.5), d, 1.0), ((hi + 0.6, 0.5, 0.5), flip(d, [3]), 2.0),          # cell 2^20 - 1: in range, and a duplicate pair there
               ((float(2 ** 20), 0.5, 0.5), flip(d, [4]), 0.5),                                    # cell 2^20: out of range, suppresses nobody
               ((0.5, -hi, 0.5), _desc(rng, 1)[0], 1.0),                                           # cell -(2^20 - 1)
               ((0.5, -hi - 0.25, 0.5), _desc(rng, 1)[0], 1.0),                                    # floor -> -2^20: out of range (truncation would keep it)
               ((0.5, 0.5, -float(2 ** 20)), _desc(rng, 1)[0], 1.0),                               # exactly -2^20
               ((0.5, 0.5, 1e300), _desc(rng, 1)[0], 1.0), ((-1e300, 0.5, 0.5), _desc(rng, 1)[0], 1.0)]
        k = _pairs(pts, 1.0)
        k["want"] = dict(out_of_range=[2, 4, 5, 6, 7], dup=[1])
        return k
    if name == "floor_negative":                                         # pairs just either side of a cell boundary at and below zero
        d = [_desc(rng, 1)[0] for _ in range(4)]
        e = 2.0 ** -40
        pts = [((-e, 0.5, 0.5), d[0], 1.0), ((e, 0.5, 0.5), flip(d[0], [1]), 2.0),                # cells -1 and 0
               ((0.5, -1.0 - e, 0.5), d[1], 2.0), ((0.5, -1.0 + e, 0.5), flip(d[1], [2]), 1.0),   # cells -2 and -1
               ((0.5, 0.5, -3.0), d[2], 1.0), ((0.5, 0.5, np.nextafter(-3.0, -4.0)), flip(d[2], [9]), 2.0),   # cells -3 and -4
               ((-0.999, -0.999, -0.999), d[3], 1.0), ((-1.001, -1.001, -1.001), flip(d[3], [200]), 3.0)]
        k = _pairs(pts, 1.0)
        k["want"] = dict(dup=[1, 2, 5, 7])
        return k
    if name == "d2_edge":                                                # r_dup = 0.5, r^2 = 0.25
        d = [_desc(rng, 1)[0] for _ in range(3)]
        pts = [((0.25, 0.0, 0.1), d[0], 1.0), ((0.75, 0.0, 0.1), flip(d[0], [7]), 2.0),           # d2 = 0.25 exactly: duplicate
               ((0.25, 0.0, 5.1), d[1], 1.0), ((0.75, 2.0 ** -27, 5.1), flip(d[1], [7]), 2.0),     # d2 = 0.25 + 2^-54, the next double: not
               ((0.25, 0.0, 9.1), d[2], 1.0), ((0.75 + 2.0 ** -53, 0.0, 9.1), flip(d[2], [7]), 2.0)]   # dx one ulp longer: not
        k = _pairs(pts, 0.5)
        k["want"] = dict(dup=[1])
        return k
    if name in ("hamming_edge", "hamming_edge_5"):
        t = 32 if name == "hamming_edge" else 5
        d = [_desc(rng, 1)[0] for _ in range(2)]
        bits = rng.permutation(256).tolist()
        pts = [((0.1, 0.1, 0.1), d[0], 1.0), ((0.12, 0.1, 0.1), flip(d[0], bits[:t]), 2.0),        # exactly dup_max_dist: duplicate
               ((3.1, 0.1, 0.1), d[1], 1.0), ((3.12, 0.1, 0.1), flip(d[1], bits[:t + 1]), 2.0)]    # one more: not
        k = _pairs(pts, 0.5, **({} if t == 32 else dict(dup_max_dist=t)))
        k["want"] = dict(dup=[1])
        return k
    if name == "straddle_face_edge_corner":                              # r_dup = 1, every pair closer than 1 and in different cells; the worse point on either side
        d = [_desc(rng, 1)[0] for _ in range(6)]
        lo, hi = 0.97, 1.03
        pts = [((lo, 0.5, 0.5), d[0], 1.0), ((hi, 0.5, 0.5), flip(d[0], [0]), 2.0),
               ((lo, 4.5, 0.5), d[1], 2.0), ((hi, 4.5, 0.5), flip(d[1], [0]), 1.0),
               ((lo, lo, 8.5), d[2], 1.0), ((hi, hi, 8.5), flip(d[2], [0]), 2.0),
               ((lo + 4, hi, 8.5), d[3], 2.0), ((hi + 4, lo, 8.5), flip(d[3], [0]), 1.0),
               ((lo, lo, lo + 12), d[4], 1.0), ((hi, hi, hi + 12), flip(d[4], [0]), 2.0),
               ((hi + 4, lo, hi + 12), d[5], 2.0), ((lo + 4, hi, lo + 12), flip(d[5], [0]), 1.0)]
        k = _pairs(pts, 1.0)
        k["want"] = dict(dup=[1, 2, 5, 6, 9, 10])
        return k
    if name == "exact_duplicate_equal_score":
        d = _desc(rng, 2)
        pts = [((0.3, 0.3, 0.3), d[0], 1.0), ((7.0, 7.0, 7.0), d[1], 0.0), ((0.3, 0.3, 0.3), d[0], 1.0), ((7.0, 7.0, 7.0), d[1], -0.0), ((0.3, 0.3, 0.3), d[0], 1.0)]
        k = _pairs(pts, 0.5)
        k["want"] = dict(dup=[2, 3, 4])                                  # the lower index wins; -0 equals +0
        return k
    if name == "chain_abc":
        d = _desc(rng, 1)[0]
        pts = [((0.05, 0.2, 0.2), d, 1.0), ((0.45, 0.2, 0.2), d, 2.0), ((0.85, 0.2, 0.2), d, 3.0)]
        k = _pairs(pts, 0.5)
        k["want"] = dict(dup=[1, 2])                                     # B by A, C by B although B goes too: only A stays
        return k
    if name == "bad_or_uncertain_next_to_good":
        d = _desc(rng, 2)
        pts = [((0.3, 0.3, 0.3), d[0], 1.0), ((0.3, 0.3, 0.3), d[0], -1.0),                         # BAD (a score < 0 would be the better one)
               ((5.3, 0.3, 0.3), d[1], 2.0), ((5.3, 0.3, NAN), d[1], 0.5), ((5.3, 0.3, 0.3), d[1], 8.0)]   # BAD, and UNCERTAIN above max_score
        k = _pairs(pts, 0.5, max_score=10.0)
        k["score"][4] = 11.0
        k["want"] = dict(dup=[], bad=[1, 3], uncertain=[4])
        return k
    if name == "crowd_65":
        return _crowd(65, 3)
    if name == "crowd_300":
        return _crowd(300, 4)
    if name == "r_dup_zero_with_duplicates":
        d = _desc(rng, 2)
        pts = [((0.3, 0.3, 0.3), d[0], 1.0), ((0.3, 0.3, 0.3), d[0], 2.0), ((1e30, -1e30, 0.0), d[1], 3.0), ((1e30, -1e30, 0.0), d[1], 3.0)]
        k = _pairs(pts, 0.0)
        k["want"] = dict(dup=[], out_of_range=[], order=[0, 1, 2, 3, 4, 5, 6, 7, 8])
        return k
    raise KeyError(name)


SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 3000, 66000)                # 3000: twelve chunks; 66000: above 65,536
NAMES = tuple("n%d" % n for n in SIZES) + (
    "n1000_score_nocov", "n1000_nodedup", "equal_scores", "low_byte_scores", "high_byte_scores", "every_byte_scores", "one_byte_each_scores", "denormal_scores",
    "signed_zero_scores", "score_from_cov", "score_given_with_cov", "no_cov_no_score", "bad_variants_score", "bad_variants_trace", "max_score_edge", "cell_range_edge",
    "floor_negative", "d2_edge", "hamming_edge", "hamming_edge_5", "straddle_face_edge_corner", "exact_duplicate_equal_score", "chain_abc", "bad_or_uncertain_next_to_good",
    "crowd_65", "crowd_300", "r_dup_zero_with_duplicates")


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    k = case(name)
    return R.build(k["X"], k["cov"], k["desc"], k["score"], **k["opt"])


def check_want(name, status, order):
    """the case's planted property against a status array and an order"""
    want = case(name)["want"]
    for f, code in (("dup", R.DUPLICATE), ("bad", R.BAD), ("uncertain", R.UNCERTAIN), ("out_of_range", R.OUT_OF_RANGE)):
        if f in want:
            assert np.nonzero(status == code)[0].tolist() == list(want[f]), (name, f, np.nonzero(status == code)[0].tolist(), want[f])
    if "order" in want:
        assert order.tolist() == list(want["order"]), (name, order.tolist())
    if "order_head" in want:
        assert order[:len(want["order_head"])].tolist() == list(want["order_head"]), name


# ------------------------------------------------------------------------------------------------ the end-to-end staging
E2E = dict(n=3000, r_dup=0.05, corner_flips=8, copy_flips=1, ratio_pct=80, max_dist=58, seed=20261021)


@functools.lru_cache(maxsize=None)
def end_to_end():
    """The reason for the feature: a map of E2E["n"] random points and descriptors, a third of them with a planted near-duplicate (moved by
    less than r_dup / 4, one descriptor bit inverted, a worse score), and a frame whose corners are the ORIGINALS of the duplicated points
    with corner_flips bits inverted (bits the copy did not invert).  On the raw map the copy sits at corner_flips + 1 bits, so the ratio
    test 100 * 8 > 80 * 9 calls every such corner AMBIGUOUS; on the built map the runner-up is a random descriptor, about 128 bits away.
    -> dict(X, cov, desc, score: the raw map; opt; corners: the frame's descriptors; orig: the map index each corner belongs to)"""
    rng = np.random.default_rng(E2E["seed"])
    n = E2E["n"]; m = n // 3
    X = rng.uniform(-20.0, 20.0, (n, 3)); d = _desc(rng, n); s = rng.uniform(0.0, 1.0, n)
    orig = np.sort(rng.permutation(n)[:m])
    Xc = X[orig] + rng.uniform(-1.0, 1.0, (m, 3)) * (E2E["r_dup"] / 8.0)       # |shift| <= sqrt(3) r_dup / 8 < r_dup / 4
    bits = np.array([rng.permutation(256)[:E2E["corner_flips"] + E2E["copy_flips"]] for _ in range(m)])
    dc = np.array([flip(d[o], b[:E2E["copy_flips"]].tolist()) for o, b in zip(orig, bits)], np.uint8)
    corners = np.array([flip(d[o], b[E2E["copy_flips"]:].tolist()) for o, b in zip(orig, bits)], np.uint8)
    Xr = np.concatenate([X, Xc]); dr = np.concatenate([d, dc]); sr = np.concatenate([s, s[orig] + 1.0])
    p = rng.permutation(len(Xr))                                              # copies and originals interleaved
    inv = np.argsort(p)
    return dict(X=Xr[p], cov=None, desc=dr[p], score=sr[p], opt=dict(r_dup=E2E["r_dup"]), corners=corners, orig=inv[orig].astype(np.int64), copy=inv[n + np.arange(m)].astype(np.int64))
