"""The case table of the guided-matching stage tests (CPU only: inputs, and for the hand-made cases the fields the contract demands).
tests/test_orb_match_ref.py holds the restatement (tests/orb_match_ref.py) to a brute-force loop and to the hand-written fields on every
case; tests/test_gpu_orb_match_stages.py runs the same cases on the GPU against the restatement - one table, so the two cannot drift."""
import functools
import numpy as np
from tests import orb_match_ref as R

W, H = 752, 480
N_CAND = (0, 1, 63, 64, 65, 4096)          # none, one (no runner-up), one short of a sweep of 64 lanes, exactly one, one more, the cap
N_Q = (1, 64, 1024)                        # one wavefront, 16 whole workgroups of four, the cap


def _case(cp, cd, qp, qr, qd, max_dist=58, ratio_pct=100, want=None):
    return dict(cand_pts=np.asarray(cp, np.float32).reshape(-1, 2), cand_desc=np.asarray(cd, np.uint8).reshape(-1, 32), q_px=np.asarray(qp, np.float32).reshape(-1, 2),
                q_radius=np.broadcast_to(np.asarray(qr, np.float32), (len(np.asarray(qp).reshape(-1, 2)),)).copy(), q_desc=np.asarray(qd, np.uint8).reshape(-1, 32),
                max_dist=max_dist, ratio_pct=ratio_pct, want=want or {})


def random_case(n_cand, n_q, seed=0):
    """corners on quarter pixels all over a 752 x 480 image; every query sits within 5 px of a corner and carries that corner's descriptor
    with 0..80 bits inverted (both sides of the 58-bit gate), radius 40: ~57 corners per window at the cap, several queries per corner"""
    rng = np.random.default_rng([20261020, n_cand, n_q, seed])
    cp = np.stack([rng.integers(4, 4 * (W - 1), n_cand), rng.integers(4, 4 * (H - 1), n_cand)], -1).astype(np.float32) / 4
    cd = rng.integers(0, 256, (n_cand, 32), dtype=np.uint8)
    if n_cand:
        src = rng.integers(0, n_cand, n_q)
        qp = cp[src] + rng.uniform(-5, 5, (n_q, 2)).astype(np.float32)
        qd = cd[src].copy()
        for i in range(n_q):
            flip = rng.choice(256, rng.integers(0, 81), replace=False)
            bits = np.unpackbits(qd[i]); bits[flip] ^= 1; qd[i] = np.packbits(bits)
    else:
        qp = rng.uniform(0, W, (n_q, 2)).astype(np.float32); qd = rng.integers(0, 256, (n_q, 32), dtype=np.uint8)
    return _case(cp, cd, qp, 40.0, qd, want=dict(second_all=-1) if n_cand == 1 else None)


def _hand_cases():
    Z = np.zeros(32, np.uint8); F = np.full(32, 255, np.uint8)
    B = R.desc_with_bits
    c = {}
    # ---- ties: 70 identical descriptors in one window (more than one sweep of 64 lanes): the lowest index, runner-up at the same distance
    pts70 = np.stack([100 + np.arange(70) % 10, 100 + np.arange(70) // 10], -1)
    c["identical_descriptors"] = _case(pts70, np.tile(B(7), (70, 1)), [[104, 103]], 50.0, [Z], want=dict(cand=[0], dist=[7], second=[7], n_window=[70], status=[R.OK]))
    # the same with the window cut: row y = 100 is outside, of row y = 101 only x = 104 (index 14) is inside, on the edge: the lowest index INSIDE wins
    c["identical_descriptors_cut"] = _case(pts70, np.tile(B(7), (70, 1)), [[104.0, 106.0]], 5.0, [Z], want=dict(cand=[14], dist=[7], second=[7], status=[R.OK]))
    # ---- the distance's range
    c["zero_vs_ones_256"] = _case([[10, 10], [12, 10]], [F, F], [[10, 10]], 5.0, [Z], max_dist=256, want=dict(cand=[0], dist=[256], second=[256], status=[R.OK]))
    c["zero_vs_ones_255"] = _case([[10, 10], [12, 10]], [F, F], [[10, 10]], 5.0, [Z], max_dist=255, want=dict(cand=[0], dist=[256], status=[R.TOO_FAR]))
    c["max_dist_0_exact"] = _case([[10, 10], [12, 10]], [B(1), B(40, 8)], [[10, 10]], 5.0, [B(40, 8)], max_dist=0, want=dict(cand=[1], dist=[0], second=[41], status=[R.OK]))
    c["max_dist_0_one_bit"] = _case([[10, 10]], [B(1)], [[10, 10]], 5.0, [Z], max_dist=0, want=dict(cand=[0], dist=[1], second=[-1], status=[R.TOO_FAR]))
    # ---- radius edges: candidates at offsets (0, 0), (3, 4), (4, 4), (-5, 0.25) from the query at (200.5, 100.25)
    q0 = np.array([200.5, 100.25]); offs = np.array([[0, 0], [3, 4], [4, 4], [-5, 0.25]])
    d4 = [B(9), B(5), B(3), B(1)]
    c["radius_0_exact_hit"] = _case(q0 + offs, d4, [q0], 0.0, [Z], want=dict(cand=[0], dist=[9], second=[-1], n_window=[1], status=[R.OK]))
    c["radius_345_edge"] = _case(q0 + offs, d4, [q0], 5.0, [Z], want=dict(cand=[1], dist=[5], second=[9], n_window=[2], status=[R.OK]))          # 9 + 16 <= 25; 32 and 25.0625 are not
    c["radius_just_under_5"] = _case(q0 + offs, d4, [q0], np.nextafter(np.float32(5), np.float32(0)), [Z], want=dict(cand=[0], n_window=[1]))
    c["radius_covers_all"] = _case(q0 + offs, d4, [q0], 1e6, [Z], want=dict(cand=[3], dist=[1], second=[3], n_window=[4], status=[R.OK]))
    c["radius_negative_is_squared"] = _case(q0 + offs, d4, [q0], -5.0, [Z], want=dict(cand=[1], n_window=[2]))
    # ---- non-finite queries: no candidate - except the infinite radius, whose square every finite distance is <= to
    nan, inf = np.nan, np.inf
    qs = [[nan, 100.25], [200.5, nan], [inf, 100.25], [200.5, -inf], [200.5, 100.25], [200.5, 100.25], [200.5, 100.25]]
    rs = [5.0, 5.0, 5.0, 5.0, nan, inf, -inf]
    c["non_finite_queries"] = _case(q0 + offs, d4, qs, rs, [Z] * 7, max_dist=256,
                                    want=dict(status=[R.NO_CANDIDATE] * 5 + [R.OK, R.CONFLICT], cand=[-1] * 5 + [3, 3], dist=[-1] * 5 + [1, 1], second=[-1] * 5 + [3, 3], n_window=[0] * 5 + [4, 4]))
    c["non_finite_candidate"] = _case([[nan, 10], [10, inf], [10, 10]], [B(0), B(0), B(2)], [[10, 10]], 1e6, [Z], want=dict(cand=[2], dist=[2], second=[-1], n_window=[1]))
    # ---- ratio test at 70 %: 100 * 35 = 70 * 50 passes, 100 * 36 > 70 * 50 does not
    c["ratio_35_50_passes"] = _case([[10, 10], [12, 10]], [B(50), B(35, 100)], [[11, 10]], 5.0, [Z], ratio_pct=70, want=dict(cand=[1], dist=[35], second=[50], status=[R.OK]))
    c["ratio_36_50_ambiguous"] = _case([[10, 10], [12, 10]], [B(50), B(36, 100)], [[11, 10]], 5.0, [Z], ratio_pct=70, want=dict(cand=[1], dist=[36], second=[50], status=[R.AMBIGUOUS]))
    c["ratio_second_0"] = _case([[10, 10], [12, 10]], [Z, Z], [[11, 10]], 5.0, [Z], ratio_pct=1, want=dict(cand=[0], dist=[0], second=[0], status=[R.OK]))
    # ---- conflicts.  Candidate 0 at (50, 50) is everybody's best at distance 4; candidate 1 at (60, 50), distance 6, is in the window of query 1 only
    two = [[50, 50], [60, 50]]
    c["conflict_two_equal"] = _case(two, [B(4), B(6)], [[49, 50], [52, 50]], [5.0, 9.0], [Z, Z],
                                    want=dict(cand=[0, 0], dist=[4, 4], second=[-1, 6], status=[R.OK, R.CONFLICT], unclaimed=[1]))
    c["conflict_three_equal"] = _case(two, [B(4), B(6)], [[52, 50], [49, 50], [50, 51]], [9.0, 5.0, 5.0], [Z, Z, Z],
                                      want=dict(cand=[0, 0, 0], status=[R.OK, R.CONFLICT, R.CONFLICT], unclaimed=[1]))
    # the smaller distance beats the lower query index
    c["conflict_smaller_dist_wins"] = _case(two, [B(4), B(6)], [[49, 50], [50, 51], [51, 50]], 5.0, [Z, B(1), B(2)],
                                            want=dict(cand=[0, 0, 0], dist=[4, 3, 2], status=[R.CONFLICT, R.CONFLICT, R.OK]))
    # a query that fails the gate claims nothing: query 0 (distance 60 > 58) must not take the candidate from query 1
    c["too_far_claims_nothing"] = _case([[50, 50]], [B(60)], [[50, 50], [50, 50]], 5.0, [Z, B(10)], want=dict(dist=[60, 50], status=[R.TOO_FAR, R.OK]))
    # 1024 queries on one candidate: distances 40 - (q % 37) for q >= 100, 58 below: the smallest distance (4) first at q = 110
    qd = np.stack([B(58 if q < 100 else 40 - q % 37) for q in range(1024)])
    st = np.full(1024, R.CONFLICT); st[110] = R.OK
    c["pile_up_1024"] = _case([[300, 200]], [Z], np.tile([[301.0, 199.0]], (1024, 1)), 3.0, qd, want=dict(cand=[0] * 1024, status=st.tolist()))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    c = {f"random_c{nc}_q{nq}": random_case(nc, nq) for nc in N_CAND for nq in N_Q}
    c.update(_hand_cases())
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's answer, computed once per session and shared (read-only)"""
    k = cases()[name]
    r = R.match(k["cand_pts"], k["cand_desc"], k["q_px"], k["q_radius"], k["q_desc"], k["max_dist"], k["ratio_pct"])
    r.setflags(write=False)
    return r


def check_want(name, res):
    """the hand-written fields of a case against a result array"""
    want = cases()[name]["want"]
    for f, v in want.items():
        if f == "second_all":
            assert (res["second"][res["n_window"] > 0] == v).all(), (name, f)
        elif f == "unclaimed":
            assert not np.isin(res["cand"], v).any(), (name, f)
        else:
            assert res[f].tolist() == list(v), (name, f, res[f].tolist())


# =========================================================================== the front-end call on a rendered stream
SEQ = "odd"                    # tests/mask_replay.py: 301 x 203 windows of the rendered frames, two pyramid levels, 80 tracks, min_distance 10
TRACK_K, TRACK_AHEAD = 20, 5   # the map is the tracks after frame 20; they are looked up in frame 25
SHIFT, RADIUS, NEAR = (3.0, -2.0), 8.0, 2.0
# share of the OK matches that land within NEAR px of the track's own position when the restatement runs on the oracle front-end's frames
# (tests/test_orb_match_ref.py measures it and holds this figure to it); the GPU must reach it minus 5 points
ORACLE_OK, ORACLE_SHARE = 29, 27.0 / 29.0          # 41 surviving map points: 29 OK (27 of them near, 93.1 %), 12 TOO_FAR; 358 corners offered


def drive(fe, frames, seq, n, after=None):
    """n frames through a front-end with .processImage-like `fe(img, ts, imu) -> (have, features)`; after(i, img) is called behind each"""
    from tests import mask_replay as MR
    out = []
    for i, (ts, img) in enumerate(frames[:n]):
        out.append(fe(img, ts, MR.imu_for(seq, ts)))
        if after:
            after(i, img)
    return out


def tracking_queries(map_tracks, cur_tracks):
    """the surviving map points' queries: -> (q_px = current pixel + SHIFT, their map descriptors, the current pixels)"""
    pos = {int(i): k for k, i in enumerate(map_tracks["ids"])}
    keep = [k for k, i in enumerate(cur_tracks["ids"]) if int(i) in pos]
    own = cur_tracks["pts"][keep]
    desc = map_tracks["desc"][[pos[int(cur_tracks["ids"][k])] for k in keep]]
    return own + np.array(SHIFT, np.float32), desc, own


def near_share(matches, own):
    ok = matches["status"] == R.OK
    d = np.linalg.norm(matches["px"][ok].astype(np.float64) - own[ok], axis=1)
    return int(ok.sum()), (float((d <= NEAR).mean()) if ok.any() else 0.0)
