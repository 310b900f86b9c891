"""CPU: the judge of the global-search GPU tests is itself judged - tests/orb_global_ref.py against a brute-force double loop over
oracle.lvo.hamming and against the fields written by hand in tests/orb_global_cases.py - and shown to tell the mistakes of a tiled kernel
apart: each mutation of the restatement changes its answer on a named case."""
import re
import os

import numpy as np
import pytest

from larvio_amd import _lib, ops
from oracle import lvo
from tests import orb_global_cases as GC
from tests import orb_global_ref as R

SMALL = [n for n, k in GC.cases().items() if len(k["map_desc"]) <= 3 * GC.S + 7]


def _brute_corner(k, c):
    """one corner by the contract's words and lvo.hamming -> (cand, dist, second, provisional status)"""
    d = [(lvo.hamming(k["cand_desc"][c], k["map_desc"][m]), m) for m in range(len(k["map_desc"]))]
    if not d:
        return -1, -1, -1, R.NO_CANDIDATE
    best = min(d)                                            # (distance, index): ties to the lowest index
    rest = [x for x, m in d if m != best[1]]
    second = min(rest) if rest else -1
    st = R.TOO_FAR if best[0] > k["max_dist"] else R.AMBIGUOUS if second >= 0 and 100 * best[0] > k["ratio_pct"] * second else R.OK
    return best[1], best[0], second, st


@pytest.mark.parametrize("name", SMALL)
def test_restatement_is_the_brute_force_loop(name):
    k = GC.cases()[name]; ref = GC.reference(name)
    best, sel, info = ref["best"], ref["sel"], ref["info"]
    nc, nm = len(k["cand_desc"]), len(k["map_desc"])
    rng = np.random.default_rng(5)
    some = range(nc) if nc * max(nm, 1) <= 70000 else sorted(rng.choice(nc, max(1, 70000 // nm), replace=False).tolist())
    for c in some:
        cand, dist, second, st = _brute_corner(k, c)
        got = best[c]
        assert (got["cand"], got["dist"], got["second"], got["n_window"]) == (cand, dist, second, nm), (name, c)
        assert (got["status"] in (R.OK, R.CONFLICT)) == (st == R.OK) and (st == R.OK or got["status"] == st), (name, c)
    # uniqueness, from the words of the contract: a provisional corner loses iff another provisional one holds a smaller (dist, corner) on its map point
    prov = [c for c in range(nc) if best["status"][c] in (R.OK, R.CONFLICT)]
    by_point = {}
    for c in prov:
        by_point.setdefault(int(best["cand"][c]), []).append((int(best["dist"][c]), c))
    for c in prov:
        lost = min(by_point[int(best["cand"][c])]) != (int(best["dist"][c]), c)
        assert best["status"][c] == (R.CONFLICT if lost else R.OK), (name, c)
    # the selection: the OK corners sorted by (dist, corner), cut at max_matches; the counts
    ok = sorted((int(best["dist"][c]), c) for c in range(nc) if best["status"][c] == R.OK)[:k["max_matches"]]
    assert [(int(r["dist"]), int(r["cand"])) for r in sel] == ok
    assert all(r["index"] == best["cand"][r["cand"]] and r["second"] == best["second"][r["cand"]] for r in sel)
    counts = [int((best["status"] == s).sum()) for s in (R.OK, R.NO_CANDIDATE, R.TOO_FAR, R.AMBIGUOUS, R.CONFLICT)]
    assert [int(info[f]) for f in ("n_ok", "n_no_candidate", "n_too_far", "n_ambiguous", "n_conflict")] == counts and sum(counts) == nc
    assert info["n_selected"] == len(sel) == min(counts[0], k["max_matches"]) and not info["pad"].any() and (best["pad"] == 0).all()


@pytest.mark.parametrize("name", list(GC.cases()))
def test_hand_written_fields(name):
    GC.check_want(name, GC.reference(name))


def test_the_cap_case_reaches_every_index_bit():
    k = GC.cases()["cap_m1048576_c8"]; best = GC.reference("cap_m1048576_c8")["best"]
    assert len(k["map_desc"]) == _lib.MAP_MAX_POINTS == 1 << 20
    got = set(best["cand"][:4].tolist())
    assert got == {0, (1 << 20) - 1, 300 * GC.S - 1, 300 * GC.S}
    for q in range(4):                                       # held to the oracle's distance on the planted pairs
        assert lvo.hamming(k["cand_desc"][q], k["map_desc"][best["cand"][q]]) == best["dist"][q] == 3
    assert (best["status"][4:] == R.TOO_FAR).all() and (best["second"] > 58).all()


def test_the_random_cases_reach_every_status():
    """the shapes are only worth running if they exercise the rules"""
    st = GC.reference(f"random_m{GC.S + 1}_c4096")["best"]["status"]
    assert {R.OK, R.TOO_FAR, R.AMBIGUOUS, R.CONFLICT} <= set(st.tolist())
    big = GC.reference(f"random_m{3 * GC.S + 7}_c4096")
    assert big["info"]["n_ok"] > big["info"]["n_selected"] == 1024          # the cut of the selection is exercised at the cap
    b = big["best"]
    assert ((b["second"] == b["dist"]) & (b["status"] != R.TOO_FAR)).any()  # ties between copies of a map point


MUTATION_CASE = {"second_from_best_slice": "best_last_slice_second_first", "ties_by_slice_order": "equal_two_slices",
                 "claims_by_corner_only": "pile_up_64", "select_in_corner_order": "more_ok_than_max_matches"}


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_each_tiling_mistake_changes_the_answer_on_its_case(mutation):
    name = MUTATION_CASE[mutation]
    k = GC.cases()[name]; ref = GC.reference(name)
    bad = R.match(k["map_desc"], k["cand_desc"], k["max_dist"], k["ratio_pct"], k["max_matches"], mutation=mutation, slice_size=GC.S)
    same = all(bad[f].tobytes() == ref[f].tobytes() for f in ("best", "sel", "info"))
    assert not same, (mutation, name)
    with pytest.raises(AssertionError):
        GC.check_want(name, bad)                             # and the hand-written fields catch it too


def test_record_layouts_and_tile_constants_match_the_library():
    assert R.GLOBAL_MATCH == _lib.GLOBAL_MATCH and R.GLOBAL_INFO == _lib.GLOBAL_INFO and R.RESULT == _lib.MATCH_RESULT
    assert _lib.GLOBAL_MATCH.itemsize == 16 and _lib.GLOBAL_INFO.itemsize == 32 and _lib.RELOC_MATCH.itemsize == 40
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "fe_global.hip")).read()
    assert int(re.search(r"#define GLB_SLICE\s+(\d+)", src).group(1)) == ops.ORB_GLOBAL_SLICE
    assert int(re.search(r"#define GLB_TILE\s+(\d+)", src).group(1)) == ops.ORB_GLOBAL_TILE
