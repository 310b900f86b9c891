"""The case table of the global-search stage tests (CPU only: inputs, and for the hand-made cases the fields the contract demands).
tests/test_orb_global_ref.py holds the restatement (tests/orb_global_ref.py) to a brute-force loop and to the hand-written fields;
tests/test_gpu_orb_global_stages.py runs the same cases on the GPU against the restatement - one table, so the two cannot drift.
S is the search kernel's slice of the map and T its tile of corners (larvio_amd.ops.ORB_GLOBAL_SLICE / ORB_GLOBAL_TILE): the shapes follow
the code."""
import functools
import numpy as np

from larvio_amd.ops import ORB_GLOBAL_SLICE as S, ORB_GLOBAL_TILE as T
from tests import orb_global_ref as R

CAP_MAP = 1 << 20


def _case(md, cd, max_dist=58, ratio_pct=100, max_matches=1024, want=None):
    return dict(map_desc=np.asarray(md, np.uint8).reshape(-1, 32), cand_desc=np.asarray(cd, np.uint8).reshape(-1, 32), max_dist=max_dist, ratio_pct=ratio_pct,
                max_matches=max_matches, want=want or {})


def n_map_values(s=S):
    return (1, 2, 63, 64, 65, s - 1, s, s + 1, 3 * s + 7)


def n_cand_values(t=T):
    return (1, 63, 65, t + 1, 4096)


def random_case(n_map, n_cand, ratio_pct=100, seed=0):
    """a random map; every corner carries the descriptor of a random map point with 0..80 bits inverted (both sides of the 58-bit gate),
    several corners per map point where there are more corners than points; every eighth map point is a copy of an earlier one, so that
    ties between indices (and, past a slice, between slices) occur"""
    rng = np.random.default_rng([20261021, n_map, n_cand, seed])
    md = rng.integers(0, 256, (n_map, 32), dtype=np.uint8)
    for i in range(8, n_map, 8):
        md[i] = md[rng.integers(0, i)]
    src = rng.integers(0, n_map, n_cand)
    cd = md[src].copy()
    for i in range(n_cand):
        flip = rng.choice(256, rng.integers(0, 81), replace=False)
        bits = np.unpackbits(cd[i]); bits[flip] ^= 1; cd[i] = np.packbits(bits)
    return _case(md, cd, ratio_pct=ratio_pct, want=dict(second_all=-1) if n_map == 1 else None)


def far(n):
    """n distinct descriptors with 150..209 bits set: far from the zero descriptor"""
    return np.stack([R.desc_with_bits(150 + i % 60, (i * 13) % 256) for i in range(n)]) if n else np.zeros((0, 32), np.uint8)


def _hand_cases(s, t):
    Z = np.zeros(32, np.uint8); F = np.full(32, 255, np.uint8)
    B = R.desc_with_bits
    c = {}
    # ---- the best in the last, partial slice, the runner-up in the first
    md = far(3 * s + 7); md[3 * s + 3] = B(5); md[2] = B(9, 40)
    c["best_last_slice_second_first"] = _case(md, [Z], want=dict(cand=[3 * s + 3], dist=[5], second=[9], status=[R.OK]))
    # ---- equal distances in two slices: the lowest index, and second == dist
    md = far(2 * s + 5); md[s - 1] = B(6); md[s + 4] = B(6, 50)
    c["equal_two_slices"] = _case(md, [Z], want=dict(cand=[s - 1], dist=[6], second=[6], status=[R.OK]))
    # ---- exact duplicates at distance 0 are not ambiguous, whatever the ratio
    md = far(65); md[10] = md[40] = B(77, 9)
    c["duplicates_dist0"] = _case(md, [B(77, 9)], ratio_pct=1, want=dict(cand=[10], dist=[0], second=[0], status=[R.OK]))
    # ---- 64 corners on one map point (the last of s + 1, behind a slice border): corner 0 is NOT the closest; (dist, corner) decides
    md = far(s + 1); md[s] = Z
    k = [30 if q < 5 else 20 - q % 7 for q in range(64)]                     # the smallest distance, 14, first at corner 6
    st = np.full(64, R.CONFLICT); st[6] = R.OK
    c["pile_up_64"] = _case(md, np.stack([B(kk, 3 * q) for q, kk in enumerate(k)]), want=dict(cand=[s] * 64, dist=k, status=st.tolist(), sel_cand=[6], sel_index=[s]))
    # ---- dist exactly at max_dist and one above
    c["max_dist_edge"] = _case([Z, F], [B(58), B(59, 100)], want=dict(cand=[0, 0], dist=[58, 59], status=[R.OK, R.TOO_FAR], sel_cand=[0]))
    c["max_dist_0"] = _case([Z, F], [Z, B(1)], max_dist=0, want=dict(dist=[0, 1], status=[R.OK, R.TOO_FAR]))
    c["max_dist_256"] = _case([F], [Z], max_dist=256, want=dict(cand=[0], dist=[256], second=[-1], status=[R.OK]))
    # ---- the ratio boundary at 70 %: 100 * 35 == 70 * 50 passes, 100 * 36 > 70 * 50 does not.  Corner 0 is Z (distance = bits set), corner 1
    # is all ones (distance = bits clear): map points 2 and 3 have 220 and 206 bits set
    c["ratio_boundary"] = _case([B(35, 100), B(50), B(220, 7), B(206, 30)], [Z, F], ratio_pct=70,
                                want=dict(cand=[0, 2], dist=[35, 36], second=[50, 50], status=[R.OK, R.AMBIGUOUS], sel_cand=[0]))
    # ---- more OK matches than max_matches, equal distances on either side of the cut: 40 corners on 40 map points of their own, distance
    # 2, 0, 2, 1 by corner % 4: ten at 0, ten at 1, twenty at 2; 25 are kept: the five lowest corners of those at distance 2
    rng = np.random.default_rng(20261022)
    md = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    kk = [(2, 0, 2, 1)[q % 4] for q in range(40)]
    cd = md.copy()
    for q in range(40):
        bits = np.unpackbits(cd[q]); bits[np.arange(kk[q]) * 5 + q] ^= 1; cd[q] = np.packbits(bits)
    by = sorted(range(40), key=lambda q: (kk[q], q))
    c["more_ok_than_max_matches"] = _case(md, cd, max_matches=25, want=dict(dist=kk, status=[R.OK] * 40, sel_cand=by[:25], n_ok=40, n_selected=25))
    c["max_matches_1"] = _case(md, cd, max_matches=1, want=dict(sel_cand=[1], n_ok=40, n_selected=1))
    # ---- no map: every corner NO_CANDIDATE
    c["n_map_0"] = _case(np.zeros((0, 32), np.uint8), far(65), want=dict(cand=[-1] * 65, dist=[-1] * 65, second=[-1] * 65, status=[R.NO_CANDIDATE] * 65, n_selected=0))
    return c


def cap_case(s=S):
    """the map's cap: 1,048,576 random points, eight corners; four of them are map points 0, 1,048,575 and the two sides of a slice border
    with a few bits inverted - the key's 20 index bits -, four are random (their best of a million random points is beyond the gate)"""
    rng = np.random.default_rng(20261023)
    md = rng.integers(0, 256, (CAP_MAP, 32), dtype=np.uint8)
    at = [0, CAP_MAP - 1, 300 * s - 1, 300 * s]
    cd = np.concatenate([md[at], rng.integers(0, 256, (4, 32), dtype=np.uint8)])
    for q in range(4):
        cd[q, q] ^= 0x07                                                       # three bits off
    return _case(md, cd, ratio_pct=80, want=dict(cand4=at, dist4=[3] * 4, status4=[R.OK] * 4))


@functools.lru_cache(maxsize=None)
def cases(s=S, t=T):
    c = {}
    for nm in n_map_values(s):
        c[f"random_m{nm}_c65"] = random_case(nm, 65, ratio_pct=100 if nm % 2 else 80)
    for nc in n_cand_values(t):
        c[f"random_m{s + 1}_c{nc}"] = random_case(s + 1, nc, ratio_pct=80)
    c[f"random_m{3 * s + 7}_c4096"] = random_case(3 * s + 7, 4096)
    c[f"random_m65_c{t + 1}"] = random_case(65, t + 1)
    c.update(_hand_cases(s, t))
    c["cap_m1048576_c8"] = cap_case(s)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's answer, computed once per session and shared (read-only)"""
    k = cases()[name]
    r = R.match(k["map_desc"], k["cand_desc"], k["max_dist"], k["ratio_pct"], k["max_matches"])
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def check_want(name, res):
    """the hand-written fields of a case against a result dict (best, sel, info)"""
    want = cases()[name]["want"]
    best, sel, info = res["best"], res["sel"], res["info"]
    for f, v in want.items():
        if f == "second_all":
            assert (best["second"] == v).all(), (name, f)
        elif f in ("sel_cand", "sel_index"):
            assert sel[f[4:]][:len(v)].tolist() == list(v), (name, f, sel[f[4:]].tolist())
        elif f in ("n_ok", "n_selected"):
            assert int(info[f]) == v, (name, f, int(info[f]))
        elif f.endswith("4"):
            assert best[f[:-1]][:4].tolist() == list(v), (name, f, best[f[:-1]][:4].tolist())
        else:
            assert best[f].tolist() == list(v), (name, f, best[f].tolist())
