"""GPU: lvk_frontend_build_map (ImageProcessor.build_map) on a rendered stream (tests/mask_replay.py's 301 x 203 cut).

same map       build_map leaves a resident map for which match_map and relocalise_map (the global search of the resident map) give the bytes
               they give after set_map with the judge's gathered arrays (tests/map_build_ref.py); map_size = n_kept; order and info are the
               judge's
refusals       a refused call leaves the previous map in place; a build that keeps nothing frees it, as set_map with no points does
end to end     the reason for the feature.  The frame's corners (tests/orb_match_ref.frame_candidates) are the observations; the map's true
               members are those corners lifted to 3D with E2E["corner_flips"] descriptor bits inverted, the rest of the few thousand points
               is random.  A third of the map gets a planted near-duplicate - every true member whose corner is at least ISOLATED bits from
               every other corner among them -: moved by less than r_dup / 4, one more bit inverted, a worse score.  On the raw map (set_map)
               every duplicated member's corner is AMBIGUOUS at ratio_pct 80 (100 * 8 > 80 * 9); on the built map every one of them is OK and
               matched to the original.  The restatements alone (tests/orb_global_ref.py, tests/map_build_ref.py) must show both before the
               GPU is relied on.

Two departures from the issue's wording, because the resident map's device buffers cannot be reached from larvio_amd.ops: the global search of
the resident map is exercised through relocalise_map (lvk_orb_match_global on the map in force, then the RANSAC) and not through
ops.orb_match_global, and the end-to-end frame is the rendered stream's, whose corners relocalise_map detects itself, not a purely synthetic
list of corner descriptors.  The issue's synthetic staging (tests/map_build_cases.end_to_end) is asserted on the CPU, with
tests/orb_global_ref.py and the judge alone, in tests/test_map_build_ref.py."""
import ctypes as C

import numpy as np
import pytest

from tests import map_build_cases as BC
from tests import map_build_ref as BR
from tests import map_select_cases as SC
from tests import mask_replay as MR
from tests import orb_global_ref as GR
from tests import orb_match_cases as MC
from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu

R_WC = SC._rot(np.random.default_rng(77)); P_WC = np.array([1.5, -0.7, 0.4])
UNIT = (1.0, 1.0, 0.0, 0.0)
ISOLATED = 48           # a duplicated member's corner is at least this far from every other corner: with 8 bits inverted on the map's side the
                        # runner-up on the built map is then at 40 or more, and 100 * 8 > 80 * 40 is false
N_MAP, R_DUP = 3000, 0.05


def _frontend(gpu_ctx, cfg):
    import larvio_amd
    gpu = larvio_amd.ImageProcessor(cfg, gpu_ctx)
    assert gpu.initialize()
    return gpu


def _step(gpu):
    def f(img, ts, imu):
        have, msg = gpu.processImage(img, imu, ts=ts)
        return msg.features.tobytes() if have else b""
    return f


@pytest.fixture(scope="module")
def stream():
    return MR.sequence(MC.SEQ)


@pytest.fixture(scope="module")
def cands(stream):
    frames, seq, cfg = stream
    return R.frame_candidates(cfg, frames[2][1])


def staged(cfg, pts, desc, seed=20261021):
    """-> dict(X, desc, score: the raw map, shuffled; dup_corner: the corners whose member is duplicated; orig / copy: the raw indices of
    their member and of its copy; member: the raw index of every corner's member)"""
    from oracle import lvo
    E = BC.E2E
    rng = np.random.default_rng(seed)
    n = len(pts)
    und = lvo.undistort(pts, cfg["intrinsics"], cfg["distortion_model"], cfg["distortion"], UNIT).astype(np.float64)
    z = rng.uniform(2.0, 9.0, n)
    X_true = np.column_stack([und * z[:, None], z]) @ R_WC.T + P_WC                    # the map is in the world frame
    bits = np.array([rng.permutation(256)[:E["corner_flips"] + E["copy_flips"]] for _ in range(N_MAP)])
    d_true = np.array([BC.flip(desc[c], bits[c][E["copy_flips"]:].tolist()) for c in range(n)], np.uint8)
    X = np.concatenate([X_true, rng.uniform(-30.0, 30.0, (N_MAP - n, 3))])
    d = np.concatenate([d_true, rng.integers(0, 256, (N_MAP - n, 32), dtype=np.uint8)])
    s = rng.uniform(0.0, 1.0, N_MAP)
    between = BR.hamming(desc[:, None, :], desc[None, :, :]) + 1000 * np.eye(n, dtype=np.int64)
    dup_corner = np.nonzero(between.min(1) >= ISOLATED)[0]
    others = n + rng.permutation(N_MAP - n)[:max(N_MAP // 3 - len(dup_corner), 0)]      # random points make the third full
    src = np.concatenate([dup_corner, others])
    Xc = X[src] + rng.uniform(-1.0, 1.0, (len(src), 3)) * (R_DUP / 8.0)
    dc = np.array([BC.flip(d[o], bits[o][:E["copy_flips"]].tolist()) for o in src], np.uint8)
    Xr = np.concatenate([X, Xc]); dr = np.concatenate([d, dc]); sr = np.concatenate([s, s[src] + 1.0])
    p = rng.permutation(len(Xr)); inv = np.argsort(p)
    return dict(X=Xr[p], desc=dr[p], score=sr[p], dup_corner=dup_corner, orig=inv[dup_corner], copy=inv[N_MAP + np.arange(len(dup_corner))], member=inv[:n],
                n_copies=len(src))


def judged(m, desc):
    """the two facts by the restatements alone -> (the judge's build, the raw search, the built search)"""
    E = BC.E2E
    raw = GR.match(m["desc"], desc, E["max_dist"], E["ratio_pct"], 1024)
    dc = m["dup_corner"]
    assert len(dc) >= 20, len(dc)
    assert (raw["best"]["status"][dc] == GR.AMBIGUOUS).all() and (raw["best"]["dist"][dc] == E["corner_flips"]).all()          # EVERY duplicated member's corner
    ref = BR.build(m["X"], None, m["desc"], m["score"], r_dup=R_DUP)
    assert ref["info"]["n_duplicate"] == m["n_copies"] and (ref["status"][m["copy"]] == BR.DUPLICATE).all() and (ref["status"][m["orig"]] == BR.KEPT).all()
    built = GR.match(ref["desc"], desc, E["max_dist"], E["ratio_pct"], 1024)
    assert (built["best"]["status"][dc] == GR.OK).all() and np.array_equal(ref["order"][built["best"]["cand"][dc]], m["orig"])  # every one of them is OK
    return ref, raw, built


def _reloc_bytes(gpu):
    res, m, info = gpu.relocalise_map(R_WC, P_WC, ratio_pct=BC.E2E["ratio_pct"], seed=5)
    return res.tobytes(), m.tobytes(), info.tobytes()


def _match_bytes(gpu):
    rec, info = gpu.match_map(R_WC, P_WC)
    return np.ascontiguousarray(rec).tobytes(), info.tobytes()


def test_build_map_is_set_map_with_the_judges_arrays_and_cures_the_duplicates(gpu_ctx, stream, cands):
    frames, seq, cfg = stream
    pts, desc = cands
    m = staged(cfg, pts, desc)
    ref, raw, built = judged(m, desc)
    dc = m["dup_corner"]
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    # ---- the raw map: every duplicated member's corner is lost to the ratio test
    gpu.set_map(m["X"], None, m["desc"])
    res, mt, info = gpu.relocalise_map(R_WC, P_WC, ratio_pct=BC.E2E["ratio_pct"], seed=5)
    assert info.tobytes() == raw["info"].tobytes() and info["n_ambiguous"] >= len(dc)
    assert not np.isin(dc, mt["cand"]).any()
    # ---- the built map
    order, binfo = gpu.build_map(m["X"], None, m["desc"], m["score"], r_dup=R_DUP)
    assert binfo.tobytes() == ref["info"].tobytes() and order.dtype == np.int32 and order.tobytes() == ref["order"].tobytes()
    assert gpu.map_size == int(ref["info"]["n_kept"]) == len(m["X"]) - m["n_copies"]
    res, mt, info = gpu.relocalise_map(R_WC, P_WC, ratio_pct=BC.E2E["ratio_pct"], seed=5)
    assert info.tobytes() == built["info"].tobytes()
    at = {int(c): int(i) for c, i in zip(mt["cand"], mt["index"])}
    assert all(int(c) in at for c in dc) and [int(order[at[int(c)]]) for c in dc] == m["orig"].tolist()      # OK, and the original
    print("end to end: %d corners, %d duplicated members; raw map n_ok %d n_ambiguous %d, built map n_ok %d n_ambiguous %d" %
          (len(pts), len(dc), raw["info"]["n_ok"], raw["info"]["n_ambiguous"], info["n_ok"], info["n_ambiguous"]))
    got = _reloc_bytes(gpu), _match_bytes(gpu)
    gpu.set_map(ref["X"], None, ref["desc"])
    assert (_reloc_bytes(gpu), _match_bytes(gpu)) == got                             # the same resident map, byte for byte in what it answers
    gpu.close()


def test_with_covariances_the_same_map_as_set_map(gpu_ctx, stream, cands):
    frames, seq, cfg = stream
    pts, desc = cands
    m = staged(cfg, pts, desc, seed=4)
    rng = np.random.default_rng(8)
    A = rng.normal(size=(len(m["X"]), 3, 3)); cov = 0.01 ** 2 * (A @ A.transpose(0, 2, 1) + 0.3 * np.eye(3))
    cov[5, 1, 1] = np.nan
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    order, info = gpu.build_map(m["X"], cov, m["desc"], r_dup=R_DUP, max_score=1.2e-3)     # the covariance's trace is the score
    ref = BR.build(m["X"], cov, m["desc"], None, r_dup=R_DUP, max_score=1.2e-3)
    assert info.tobytes() == ref["info"].tobytes() and order.tobytes() == ref["order"].tobytes() and gpu.map_size == len(order)
    assert info["n_bad"] == 1 and info["n_uncertain"] > 0 and info["n_duplicate"] > 0 and info["n_kept"] > 500
    got = _reloc_bytes(gpu), _match_bytes(gpu)
    gpu.set_map(ref["X"], ref["cov"], ref["desc"])
    assert (_reloc_bytes(gpu), _match_bytes(gpu)) == got
    gpu.close()


def test_a_refused_call_leaves_the_previous_map(gpu_ctx, stream, cands):
    import larvio_amd
    from larvio_amd._lib import lib, _p, MAP_BUILD_INFO
    frames, seq, cfg = stream
    pts, desc = cands
    m = staged(cfg, pts, desc, seed=6)
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    order, info = gpu.build_map(m["X"], None, m["desc"], m["score"], r_dup=R_DUP)
    n_kept = gpu.map_size
    good = _reloc_bytes(gpu), _match_bytes(gpu)
    few = m["X"][:10]
    for kw in (dict(max_score=-1.0), dict(r_dup=float("nan")), dict(dup_max_dist=300)):
        with pytest.raises(larvio_amd.LvkError):                                     # the wrapper raises on a refusal ...
            gpu.build_map(few, None, m["desc"][:10], **kw)
    X = np.ascontiguousarray(m["X"]); d = np.ascontiguousarray(m["desc"]); out = np.zeros(8, np.int32); bi = np.zeros(1, MAP_BUILD_INFO)
    from larvio_amd import ops
    raw = lambda n, h_desc, cap, opt=None: lib().lvk_frontend_build_map(gpu._h, _p(X), None, h_desc, None, n, C.byref(opt) if opt is not None else None, _p(out), cap, _p(bi))
    O = ops.map_build_options
    assert raw(10, _p(d), 8, O(max_score=-1.0)) == 1 and raw(10, _p(d), 8, O(r_dup=float("nan"))) == 1 and raw(10, _p(d), 8, O(dup_max_dist=300)) == 1   # ... and the code is LVK_ERR_ARG
    assert raw(len(X), _p(d), 8) == 3 and not out.any()                              # LVK_ERR_CAPACITY: room for 8 indices, more are kept
    assert raw(len(X), None, 8) == 1 and raw(-1, _p(d), 8) == 1 and raw(8, _p(d), -1) == 1 and raw((1 << 20) + 1, _p(d), 8) == 3
    assert gpu.map_size == n_kept and (_reloc_bytes(gpu), _match_bytes(gpu)) == good  # the map in force stayed, and the handle goes on
    assert raw(8, _p(d), 8) == 0 and gpu.map_size == 8 and sorted(out.tolist()) == list(range(8))   # no options: nothing culled, the order is the index order
    bad = few.copy(); bad[:, 0] = np.nan
    order, info = gpu.build_map(bad, None, m["desc"][:10])                           # nothing is kept: the map is freed
    assert len(order) == 0 and info["n_bad"] == 10 and gpu.map_size == 0
    order, info = gpu.build_map(None, None, None)
    assert len(order) == 0 and not info["n_kept"] and gpu.map_size == 0
    MC.drive(_step(gpu), frames[3:], seq, 3)
    assert gpu.state == 3
    gpu.close()
