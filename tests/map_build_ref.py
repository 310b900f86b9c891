"""The map build (lvk_map_build) restated in plain numpy from the contract in include/lvk_c.h.  There is no reference counterpart, so this
restatement is the judge of the GPU tests; tests/test_map_build_ref.py holds it to a plain Python loop over all pairs first.  Every
expression is an elementwise FP64 one in the header's order (numpy does not contract them).

    score      score[i] if given, else (c00 + c11) + c22, else 0; -0 -> +0
    cell       floor(X / r_dup) per axis when r_dup > 0
    status     BAD (non-finite X / covariance / score, negative covariance diagonal, score < 0), UNCERTAIN (score > max_score),
               OUT_OF_RANGE (r_dup > 0 and some |cell| > 2^20 - 1), DUPLICATE, KEPT
    duplicate  eligible i with an eligible j != i: (score_j, j) < (score_i, i), cells at most 1 apart on every axis,
               (dx dx + dy dy) + dz dz <= r_dup r_dup, Hamming <= dup_max_dist - whether or not j is a DUPLICATE itself
    order      the KEPT points by (score, index)

The duplicate rule is vectorised over the cell neighbourhood: the eligible points sorted by packed cell key, and for each of the 27 offsets
the run of points in that cell found by two searchsorted calls."""
import numpy as np

KEPT, BAD, UNCERTAIN, OUT_OF_RANGE, DUPLICATE = 0, 1, 2, 3, 4
INFO = np.dtype([("n_kept", np.int32), ("n_bad", np.int32), ("n_uncertain", np.int32), ("n_out_of_range", np.int32), ("n_duplicate", np.int32), ("pad", np.int32, 3)])
CELL_MAX = float(2 ** 20 - 1)
_POP = np.array([bin(v).count("1") for v in range(256)], np.int64)


def options(max_score=0.0, r_dup=0.0, dup_max_dist=0):
    """the options with the header's defaults filled in"""
    return dict(max_score=float(max_score) if max_score != 0 else np.inf, r_dup=float(r_dup), dup_max_dist=int(dup_max_dist) if dup_max_dist != 0 else 32)


def hamming(a, b):
    """Hamming distance of descriptor rows a and b (broadcast), uint8 (..., 32)"""
    return _POP[np.bitwise_xor(a, b)].sum(-1)


def classify(X, cov, score, opt):
    """-> (score (n,) with -0 canonicalised, status (n,) without the duplicate rule, cells (n, 3) float64 or None)"""
    X = np.asarray(X, np.float64).reshape(-1, 3); n = len(X)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(X).all(1)
        s = np.zeros(n)
        if cov is not None:
            c = np.asarray(cov, np.float64).reshape(n, 9)
            bad |= ~np.isfinite(c).all(1)
            bad |= (c[:, 0] < 0.0) | (c[:, 4] < 0.0) | (c[:, 8] < 0.0)
            s = (c[:, 0] + c[:, 4]) + c[:, 8]
        if score is not None:
            s = np.asarray(score, np.float64).reshape(n).copy()
        bad |= ~np.isfinite(s) | (s < 0.0)
        s = np.where(s == 0.0, 0.0, s)                                   # -0 -> +0
        status = np.full(n, KEPT, np.uint8)
        status[bad] = BAD
        status[~bad & (s > opt["max_score"])] = UNCERTAIN
        cells = None
        if opt["r_dup"] > 0.0:
            cells = np.floor(X / opt["r_dup"])
            far = (np.abs(cells) > CELL_MAX).any(1)
            status[(status == KEPT) & far] = OUT_OF_RANGE
    return s, status, cells


def duplicates(X, desc, s, status, cells, opt):
    """-> bool (n,): the eligible points the duplicate rule drops"""
    n = len(X)
    dup = np.zeros(n, bool)
    el = np.nonzero(status == KEPT)[0]
    if cells is None or len(el) < 2:
        return dup
    c = cells[el].astype(np.int64) + (1 << 20)                           # 1 .. 2^21 - 1 per axis
    key = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
    srt = np.argsort(key, kind="stable"); sk = key[srt]
    r2 = opt["r_dup"] * opt["r_dup"]
    Xe, de, se = X[el], np.asarray(desc, np.uint8).reshape(n, 32)[el], s[el]
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                q = c + np.array([ox, oy, oz])
                ok = ((q >= 1) & (q <= (1 << 21) - 1)).all(1)
                nk = (q[:, 2] << 42) | (q[:, 1] << 21) | q[:, 0]
                lo = np.searchsorted(sk, nk, "left"); hi = np.searchsorted(sk, nk, "right")
                cnt = np.where(ok, hi - lo, 0)
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                i = np.repeat(np.arange(len(el)), cnt)
                start = np.repeat(np.cumsum(cnt) - cnt, cnt)
                j = srt[np.repeat(lo, cnt) + (np.arange(tot) - start)]
                d = Xe[i] - Xe[j]
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                hit = (i != j) & (d2 <= r2)
                i, j = i[hit], j[hit]
                hit = hamming(de[i], de[j]) <= opt["dup_max_dist"]
                i, j = i[hit], j[hit]
                hit = (se[j] < se[i]) | ((se[j] == se[i]) & (el[j] < el[i]))
                dup[el[i[hit]]] = True
    return dup


def build(X, cov, desc, score=None, **opt):
    """-> dict(score, status (n,) uint8, order (n_kept,) int32, X, cov, desc: the gathered arrays (None where the input is), info: one INFO record)"""
    o = options(**opt)
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3); n = len(X)
    cv = None if cov is None else np.ascontiguousarray(cov, np.float64).reshape(n, 3, 3)
    ds = None if desc is None else np.ascontiguousarray(desc, np.uint8).reshape(n, 32)
    s, status, cells = classify(X, cv, score, o)
    status[duplicates(X, ds, s, status, cells, o)] = DUPLICATE
    kept = np.nonzero(status == KEPT)[0]
    order = kept[np.argsort(s[kept], kind="stable")].astype(np.int32)    # ties stay in index order
    info = np.zeros(1, INFO)[0]
    for f, code in (("n_kept", KEPT), ("n_bad", BAD), ("n_uncertain", UNCERTAIN), ("n_out_of_range", OUT_OF_RANGE), ("n_duplicate", DUPLICATE)):
        info[f] = int((status == code).sum())
    return dict(score=s, status=status, order=order, X=X[order], cov=None if cv is None else cv[order], desc=None if ds is None else ds[order], info=info)


def build_loops(X, cov, desc, score=None, **opt):
    """the same contract as a plain Python loop, brute force over all pairs: what tests/test_map_build_ref.py holds `build` to.  -> (status, order)"""
    import math
    o = options(**opt)
    X = np.asarray(X, np.float64).reshape(-1, 3); n = len(X)
    r = o["r_dup"]
    sc, st, cell = [0.0] * n, [KEPT] * n, [None] * n
    with np.errstate(all="ignore"):
        for i in range(n):
            vals = [float(v) for v in X[i]]
            s = 0.0
            bad = False
            if cov is not None:
                c = [float(v) for v in np.asarray(cov[i], np.float64).reshape(9)]
                vals += c
                bad = c[0] < 0 or c[4] < 0 or c[8] < 0
                s = float((np.float64(c[0]) + np.float64(c[4])) + np.float64(c[8]))
            if score is not None:
                s = float(score[i])
            bad = bad or not all(math.isfinite(v) for v in vals) or not math.isfinite(s) or s < 0
            sc[i] = 0.0 if s == 0 else s
            if bad:
                st[i] = BAD
            elif s > o["max_score"]:
                st[i] = UNCERTAIN
            elif r > 0:
                cell[i] = [math.floor(float(np.float64(v) / np.float64(r))) if math.isfinite(float(np.float64(v) / np.float64(r))) else math.inf for v in vals[:3]]
                if any(abs(v) > 2 ** 20 - 1 for v in cell[i]):
                    st[i] = OUT_OF_RANGE
    elig = [i for i in range(n) if st[i] == KEPT]
    out = list(st)
    if r > 0:
        r2 = np.float64(r) * np.float64(r)
        D = np.asarray(desc, np.uint8).reshape(n, 32)
        for i in elig:
            for j in elig:
                if j == i or not (sc[j], j) < (sc[i], i):
                    continue
                if any(abs(cell[i][a] - cell[j][a]) > 1 for a in range(3)):
                    continue
                dx, dy, dz = (np.float64(X[i][a]) - np.float64(X[j][a]) for a in range(3))
                if not ((dx * dx + dy * dy) + dz * dz <= r2):
                    continue
                if sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(D[i], D[j])) <= o["dup_max_dist"]:
                    out[i] = DUPLICATE
                    break
    kept = sorted((i for i in range(n) if out[i] == KEPT), key=lambda i: (sc[i], i))
    return np.array(out, np.uint8), np.array(kept, np.int32)
