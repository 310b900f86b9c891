"""The CPU half of the fundamental-matrix stage tests: every case of tests/fm_cases.py meets, on the oracle and on the replay of the subset
draws, the condition it was built for (a case that stops reaching its path fails here, not silently on the GPU), the replay itself agrees
with the oracle, and no reachable (n, inliers) pair puts RANSACUpdateNumIters next to a rounding edge where two math libraries could
disagree about an iteration count."""
import numpy as np
import pytest
from oracle import lvo
from tests import fm_cases as K


@pytest.mark.parametrize("name", list(K.CASES))
def test_case_meets_its_condition(name):
    K.check_case(name)


def test_every_path_has_a_case():
    paths = {c["path"] for c in K.CASES.values()}
    for p in ("table overrun, 256 threads", "table overrun, 512 threads", "iteration cap", "cap with no usable model", "collinear fallback in round 0",
              "collinear fallback in a later round", "getSubset fails at once", "window misfit", "degenerate: frozen camera", "LMedS on exact data",
              "defaults", "workgroup width edge", "capacity"):
        assert p in paths, p
    assert all(c["n"] <= K.FM_MAX_N for c in map(K.case, K.CASES))


def test_replay_draws_the_subsets_the_oracle_draws():
    """max_iters = k stops the oracle after k hypotheses; the mask it leaves is the best of the first k subsets of the replay, scored as
    test_oracle_frontend._replay_ransac scores them.  Checked where the replay's collinear redraws matter: the round-0 collinear case."""
    from tests.test_oracle_frontend import _replay_ransac
    c = K.case("collinear_round0_n40")
    for k in (1, 2, 3):
        ok, mask, iters = lvo.ransac_fundamental(c["p1"], c["p2"], 1.0, 0.99, k)
        want, it = _replay_ransac(c["p1"], c["p2"], max_iters=k)
        assert iters == it == k and np.array_equal(mask.astype(bool), want)
    rec = K.replay_draws(c["n"], 3, c["p1"], c["p2"])
    assert rec[1]["collinear"][0] and len(rec[1]["draws"]) >= 2 and rec[2]["start"] == rec[1]["start"] + sum(rec[1]["draws"])


def test_first_fallback_on_hand_made_records():
    rec = lambda starts_draws, bad=(): [dict(start=s, draws=[d], collinear=[i in bad], idx=[]) for i, (s, d) in enumerate(starts_draws)]
    seq = lambda ds: list(zip(np.concatenate([[0], np.cumsum(ds)[:-1]]).tolist(), ds))
    assert K.first_fallback(rec(seq([7] * 40))) is None
    assert K.first_fallback(rec(seq([7] * 40), bad={1})) == ("collinear", 0, 1)
    assert K.first_fallback(rec(seq([7] * 40), bad={8})) == ("collinear", 2, 8)
    assert K.first_fallback(rec(seq([7] * 8 + [16] * 16))) is None                       # 256 draws: fits exactly
    assert K.first_fallback(rec(seq([7] * 8 + [16] * 15 + [17]))) == ("window", 2, 23)
    assert K.first_fallback(rec(seq([7] * 8 + [16] * 16 + [7] * 16))) is None
    many = seq([7] * 8 + [16] * 16 * 15 + [16] * 16)                                     # round 16 + 2 starts at draw 56 + 15 * 256 = 3896 > 4096 - 256
    assert K.first_fallback(rec(many)) == ("table", 17, 8 + 16 * 15)
    assert [K.round_up(i) for i in (0, 1, 2, 3, 8, 9, 24, 25)] == [2, 2, 2, 8, 8, 24, 24, 40]


# the (n, inliers) pairs at conf = 0.99 on which device and host may legitimately disagree about an iteration count: none
HALF_INTEGER_PAIRS = []
CAP_EDGE_PAIRS = []


def test_iteration_rule_stays_clear_of_rounding_edges():
    """d_ransac_iter_rule goes through pow, log and rint; every `iterations equal` assertion rests on q = log(1 - conf) / log(1 - (g / n)^7) not
    sitting next to a half-integer, and on the cap comparison -log(1 - conf) >= 1000 * -log(denom) not sitting on equality.  In long double,
    for conf = 0.99 (what the front-end and the tests pass), every n in 8..4096 and every inlier count g in 7..n - 1 (g = n: denom is 0, the
    `zero` branch): collect the pairs within a relative 2^-30 of either edge - seven orders of magnitude more than a double libm's error.
    The half-integer edge is looked for where the rounded quotient can be used at all: q up to the cap of 1000 (d_ransac_iter_apply returns
    the bound it was given, never rint(q), once q reaches that bound; a q of 1e15 is within 2^-30 q of anything and is never rounded into a
    count).  The bound the comparison sees later in a call is an earlier q, rounded: the comparison then decides between that integer k and
    rint(q) for q next to k, which are the same number."""
    LD = np.longdouble
    tol = LD(2.0) ** -30
    num = np.log(LD(1.0 - 0.99))                                               # the double the code forms, then exact
    half, cap = [], []
    for n in range(8, K.FM_MAX_N + 1):
        g = np.arange(7, n, dtype=np.int64)
        w = (g.astype(LD) / LD(n)) ** 7
        den = np.log1p(-w)
        q = num / den
        frac = np.abs(q - (np.floor(q) + LD(0.5)))
        used = q <= LD(1000) * (1 + tol)                                       # beyond the cap the comparison keeps the bound: rint(q) is not looked at
        for gi in g[used & (frac <= tol * q)]:
            half.append((n, int(gi)))
        for gi in g[np.abs(-num - LD(1000) * -den) <= tol * -num]:
            cap.append((n, int(gi)))
    print("pairs next to a half-integer:", half, "next to the cap:", cap)
    assert half == HALF_INTEGER_PAIRS
    assert cap == CAP_EDGE_PAIRS
