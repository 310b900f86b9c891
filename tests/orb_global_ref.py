"""Global ORB search of a map (lvk_orb_match_global) restated in plain numpy from the contract in include/lvk_c.h.  There is no reference
counterpart, so this restatement is the judge of the GPU tests; tests/test_orb_global_ref.py holds it to a brute-force double loop over
oracle.lvo.hamming first, and shows that it tells the mistakes of a tiled kernel apart (the `mutation` argument makes them on purpose).

    best       per corner the map point with the smallest Hamming distance, ties to the lowest map index; second = the smallest distance
               over the other map points, -1 when there is none
    status     NO_CANDIDATE (n_map == 0; cand = dist = second = -1), TOO_FAR (dist > max_dist), AMBIGUOUS (second >= 0 and
               100 dist > ratio_pct second), else provisional; per claimed map point the smallest (dist, corner) is OK, the rest CONFLICT
    selection  the OK corners by (dist, corner), the first min(n_ok, max_matches) of them: (corner, map index, dist, second)"""
import numpy as np

from tests.orb_match_ref import hamming_rows, desc_with_bits, OK, NO_CANDIDATE, TOO_FAR, AMBIGUOUS, CONFLICT, RESULT  # noqa: F401

GLOBAL_MATCH = np.dtype([("cand", np.int32), ("index", np.int32), ("dist", np.int32), ("second", np.int32)])
GLOBAL_INFO = np.dtype([("n_ok", np.int32), ("n_no_candidate", np.int32), ("n_too_far", np.int32), ("n_ambiguous", np.int32), ("n_conflict", np.int32),
                        ("n_selected", np.int32), ("pad", np.int32, 2)])
MUTATIONS = ("second_from_best_slice", "ties_by_slice_order", "claims_by_corner_only", "select_in_corner_order")


def best_two(d, mutation=None, slice_size=None):
    """(best index, its distance, the runner-up's distance or -1) of one corner's distances d to every map point"""
    n = len(d)
    if mutation == "ties_by_slice_order" and slice_size:            # the LAST slice wins a tie between slices
        order = np.concatenate([np.arange(s, min(s + slice_size, n)) for s in range(0, n, slice_size)][::-1])
        b = int(order[np.argmin(d[order])])
    else:
        b = int(np.argmin(d))                                        # the first minimum: the lowest map index
    if mutation == "second_from_best_slice" and slice_size:
        lo = b // slice_size * slice_size
        others = np.delete(d[lo:lo + slice_size], b - lo)
    else:
        others = np.delete(d, b)
    return b, int(d[b]), int(others.min()) if len(others) else -1


def match(map_desc, cand_desc, max_dist=58, ratio_pct=100, max_matches=1024, mutation=None, slice_size=None):
    """-> dict(best: RESULT array, one record per corner; sel: the n_selected GLOBAL_MATCH records; info: one GLOBAL_INFO record)"""
    md = np.asarray(map_desc, np.uint8).reshape(-1, 32); cd = np.asarray(cand_desc, np.uint8).reshape(-1, 32)
    n_map, n_cand = len(md), len(cd)
    best = np.zeros(n_cand, RESULT)
    best["n_window"] = n_map
    for c in range(n_cand):
        r = best[c]
        if n_map == 0:
            r["cand"] = r["dist"] = r["second"] = -1; r["status"] = NO_CANDIDATE
            continue
        b, dist, second = best_two(hamming_rows(md, cd[c]), mutation, slice_size)
        r["cand"], r["dist"], r["second"] = b, dist, second
        if dist > max_dist:
            r["status"] = TOO_FAR
        elif second >= 0 and 100 * dist > ratio_pct * second:
            r["status"] = AMBIGUOUS
        else:
            r["status"] = OK                                         # provisional
    prov = np.nonzero(best["status"] == OK)[0]
    for m in np.unique(best["cand"][prov]):
        claim = prov[best["cand"][prov] == m]
        key = (lambda c: int(c)) if mutation == "claims_by_corner_only" else (lambda c: (int(best["dist"][c]), int(c)))
        win = min(claim, key=key)
        best["status"][claim[claim != win]] = CONFLICT
    ok = np.nonzero(best["status"] == OK)[0]
    order = ok if mutation == "select_in_corner_order" else ok[np.lexsort((ok, best["dist"][ok]))]
    order = order[:max_matches]
    sel = np.zeros(len(order), GLOBAL_MATCH)
    sel["cand"] = order; sel["index"] = best["cand"][order]; sel["dist"] = best["dist"][order]; sel["second"] = best["second"][order]
    info = np.zeros(1, GLOBAL_INFO)[0]
    for f, s in (("n_ok", OK), ("n_no_candidate", NO_CANDIDATE), ("n_too_far", TOO_FAR), ("n_ambiguous", AMBIGUOUS), ("n_conflict", CONFLICT)):
        info[f] = int((best["status"] == s).sum())
    info["n_selected"] = len(order)
    return dict(best=best, sel=sel, info=info)
