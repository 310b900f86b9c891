"""CPU: the judge of the map build's GPU tests (tests/map_build_ref.build) held to a plain Python loop that is brute force over all pairs
(tests/map_build_ref.build_loops), on every case of tests/map_build_cases.py with n <= 600; each case's planted property ("exactly these
indices are DUPLICATE"); and the end-to-end staging judged by tests/orb_global_ref.py alone: on the raw map every duplicated point's corner
is AMBIGUOUS at ratio_pct 80, on the judge's built map every one of them is OK."""
import numpy as np
import pytest

from tests import map_build_cases as MC
from tests import map_build_ref as R
from tests import orb_global_ref as GR

SMALL = [name for name in MC.NAMES if len(MC.case(name)["X"]) <= 600]


def test_the_case_list_covers_the_sizes():
    sizes = {len(MC.case(name)["X"]) for name in MC.NAMES}
    assert {0, 1, 2, 63, 64, 65, 255, 256, 257}.issubset(sizes) and any(1024 < s < 65536 for s in sizes) and any(s > 65536 for s in sizes)
    assert len(SMALL) >= 25


@pytest.mark.parametrize("name", SMALL)
def test_restatement_is_the_loop(name):
    k = MC.case(name); ref = MC.reference(name)
    status, order = R.build_loops(k["X"], k["cov"], k["desc"], k["score"], **k["opt"])
    assert np.array_equal(status, ref["status"]), np.nonzero(status != ref["status"])[0][:8]
    assert np.array_equal(order, ref["order"])


@pytest.mark.parametrize("name", MC.NAMES)
def test_planted_property_and_shape_of_the_answer(name):
    k = MC.case(name); ref = MC.reference(name)
    n = len(k["X"])
    MC.check_want(name, ref["status"], ref["order"])
    info = ref["info"]
    assert info["n_kept"] + info["n_bad"] + info["n_uncertain"] + info["n_out_of_range"] + info["n_duplicate"] == n and not info["pad"].any()
    assert len(ref["order"]) == info["n_kept"] and (ref["status"][ref["order"]] == R.KEPT).all()
    s = ref["score"][ref["order"]]
    assert (np.diff(s) >= 0).all() and not np.signbit(s).any()                            # ascending, and no -0 left
    tie = np.diff(s) == 0
    assert (np.diff(ref["order"])[tie] > 0).all()                                         # equal scores in index order
    assert ref["X"].tobytes() == np.ascontiguousarray(k["X"], np.float64)[ref["order"]].tobytes()
    if name in ("n3000", "n66000", "score_from_cov"):
        assert info["n_duplicate"] > 0 and info["n_bad"] == 1                              # planted copies are found (those whose pair is eligible on both sides)


def test_sorting_the_bits_is_sorting_the_values():
    """what the device sort relies on: non-negative finite doubles, -0 canonicalised, order as their bit patterns"""
    for name in ("every_byte_scores", "denormal_scores", "signed_zero_scores", "high_byte_scores", "low_byte_scores", "one_byte_each_scores"):
        ref = MC.reference(name)
        kept = np.nonzero(ref["status"] == R.KEPT)[0]
        bits = ref["score"][kept].view(np.uint64)
        assert np.array_equal(kept[np.argsort(bits, kind="stable")], ref["order"]), name
    raw = MC.case("signed_zero_scores")["score"]
    assert np.signbit(raw).any() and not np.array_equal(np.argsort(raw.view(np.uint64), kind="stable"), MC.reference("signed_zero_scores")["order"])   # the raw bits would misplace -0


def test_neighbourhood_equals_all_pairs_on_a_multi_chunk_case():
    """the vectorised duplicate rule against an all-pairs numpy one at 3000 points (the loop is too slow there)"""
    k = MC.case("n3000"); ref = MC.reference("n3000")
    o = R.options(**k["opt"])
    s, status, cells = R.classify(k["X"], k["cov"], k["score"], o)
    el = np.nonzero(status == R.KEPT)[0]
    X, d = k["X"][el], k["desc"][el]
    dup = np.zeros(len(el), bool)
    for a in range(len(el)):
        df = X[a] - X
        d2 = (df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
        near = (np.abs(cells[el] - cells[el[a]]) <= 1).all(1) & (d2 <= o["r_dup"] * o["r_dup"]) & (np.arange(len(el)) != a)
        near &= (s[el] < s[el[a]]) | ((s[el] == s[el[a]]) & (el < el[a]))
        j = np.nonzero(near)[0]
        dup[a] = bool(len(j)) and bool((R.hamming(d[j], d[a]) <= o["dup_max_dist"]).any())
    assert np.array_equal(np.sort(el[dup]), np.nonzero(ref["status"] == R.DUPLICATE)[0])


def test_end_to_end_staging_on_the_cpu():
    """the flip counts of MC.E2E do what the GPU test relies on, by the global search's restatement alone"""
    e = MC.end_to_end(); E = MC.E2E
    raw = GR.match(e["desc"], e["corners"], E["max_dist"], E["ratio_pct"], 1024)
    assert np.array_equal(raw["best"]["cand"], e["orig"]) and (raw["best"]["dist"] == E["corner_flips"]).all()
    assert (raw["best"]["second"] == E["corner_flips"] + E["copy_flips"]).all()
    assert (raw["best"]["status"] == GR.AMBIGUOUS).all() and raw["info"]["n_ok"] == 0              # EVERY duplicated point's corner
    ref = R.build(e["X"], e["cov"], e["desc"], e["score"], **e["opt"])
    assert np.array_equal(np.nonzero(ref["status"] == R.DUPLICATE)[0], np.sort(e["copy"])) and ref["info"]["n_kept"] == E["n"]
    built = GR.match(ref["desc"], e["corners"], E["max_dist"], E["ratio_pct"], 1024)
    assert (built["best"]["status"] == GR.OK).all()                                                 # every one of them is OK
    assert np.array_equal(ref["order"][built["best"]["cand"]], e["orig"])                           # and is the original, not the copy
