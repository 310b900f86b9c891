"""GPU: lvk_frontend_merge_map (ImageProcessor.merge_map) on the two synthetic sessions of tests/align3d_cases.sessions - A: 300 points; B: 120
of them seen again under yaw 0.7 rad and a (3, -2, 0.4) m shift with 1 cm of noise, plus 80 new points - on a front-end that has processed
frames of the rendered stream (tests/mask_replay.py's 301 x 203 cut), against larvio_amd.localize.merge_maps.

found      with align = None: the map's size, the order, the build's and the search's counts, the alignment's discrete fields and its winner
           (c0, s0, t0) are the judge's exactly; the refined c, s, t lie inside the refinement's bound (tests/align3d_ref.bounds).  The
           resident arrays cannot be read back directly: match_map from a camera that sees the whole site answers for them, against
           set_map with the judge's arrays - the same points in the same cells with the same match status, the float32 pixels, radii
           and depths within the refinement's bound pushed through the transform and the projection (derived in the test from
           bounds()["model"], the sessions' extent and the camera) plus the one float32 spacing by which two doubles that close can
           round apart
given      with align = the inverse of the generating A -> B alignment: everything bit for bit, match_map's bytes included
no overlap a B without a shared point: LVK_OK, a status other than ALIGN_OK, the map in force answering with the bytes it gave before
refusals   each leaves the map in force; n_A + n over the cap is refused on the counts alone, nothing that large is uploaded; a call
           between lvk_frontend_begin and the lvk_frontend_process of the same frame is refused with nothing written, and the frame's
           own process call then goes on
frames     a run with merges between frames publishes the bytes of a run without them"""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import localize as L
from larvio_amd import ops
from tests import align3d_cases as C3
from tests import align3d_ref as R3
from tests import mask_replay as MR
from tests import orb_match_cases as MC
from tests.align_cases import LEVEL

pytestmark = pytest.mark.gpu

R_WC, P_WC = LEVEL, np.array([-100.0, 0.0, 0.0])        # looks along world x from 100 m out: the whole site is in front of it
P = C3.SESSIONS


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
def judged():
    S = C3.sessions()
    return S, L.merge_maps(S["A"], S["B"], r_dup=P["r_dup"], seed=7)


def _match(gpu):
    rec, info = gpu.match_map(R_WC, P_WC)
    return np.ascontiguousarray(rec), info


def test_found_alignment_merges_as_the_judge_does(gpu_ctx, stream, judged):
    frames, seq, cfg = stream
    S, m = judged
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    gpu.set_map(*S["A"])
    used, order, info, minfo = gpu.merge_map(*S["B"], r_dup=P["r_dup"], seed=7)
    al = m["align"]
    assert used["status"] == al["status"] == R3.OK and (used["hyp"], used["n_inliers"], used["root"], used["iters"]) == (al["hyp"], al["n_inliers"], 0, 0)
    assert (used["pair_i"], used["pair_j"]) == tuple(m["pairs"][al["hyp"]])
    assert minfo.tobytes() == m["match_info"].tobytes() and info.tobytes() == m["info"].tobytes()
    assert order.dtype == np.int32 and order.tobytes() == m["order"].tobytes() and gpu.map_size == len(order) == P["n_a"] + P["n_new"]
    assert np.array([used["c0"], used["s0"], *used["t0"]]).tobytes() == np.array([al["c0"], al["s0"], *al["t0"]]).tobytes()
    ref = R3.run(m["matches_X"], m["matches_Y"], m["pairs"], None, "ld"); bnd = R3.bounds(m["matches_X"], m["matches_Y"], m["pairs"], ref)
    got = np.array([used["c"], used["s"], *used["t"]], R3.LD); want = np.array([ref["model"][0], ref["model"][1], *ref["model"][2]], R3.LD)
    print("refined model |error| / bound:", (np.abs(got - want) / bnd["model"]).astype(float))
    assert np.all(np.abs(got - want) <= bnd["model"])
    assert np.all(np.abs(used["A"].astype(R3.LD) - ref["A"]) <= bnd["A"]) and abs(R3.LD(used["rms"]) - ref["rms"]) <= bnd["rms"]
    rec, minf = _match(gpu)
    gpu.set_map(m["X"], m["cov"], m["desc"])
    rec2, minf2 = _match(gpu)
    assert minf.tobytes() == minf2.tobytes() and minf["n_selected"] >= 50, minf
    for f in ("index", "cell"):
        assert np.array_equal(rec[f], rec2[f]), f
    assert np.array_equal(rec["m"]["status"], rec2["m"]["status"])
    # the refinement's bound pushed through the transform and the projection.  A point of B moves by at most
    # dp = (|dc| + |ds|) (|X_x| + |X_y|) + max |dt|, its covariance (Rz Sigma Rz^T, entries below tr Sigma) by 4 (|dc| + |ds|) tr Sigma.  A
    # pixel is f (x / z) through a distortion whose gain stays below 2 inside the view, and |x / z| < 1 there: d px <= 4 f dp / z_min; the
    # depth moves by dp; the radius is k_sigma sqrt(lambda + sigma_px^2) >= k_sigma sigma_px with lambda <= (f / z)^2 tr Sigma, so
    # d radius <= k_sigma d lambda / (2 sigma_px), d lambda <= (f / z_min)^2 (4 (|dc| + |ds|) tr Sigma + 2 tr Sigma dp / z_min), k_sigma = 3,
    # sigma_px = 1 (the defaults).  Each value is then rounded to float32 once: two doubles that close round to the same float32 or to
    # neighbours, one spacing apart
    b = 2 * bnd["model"].astype(np.float64)               # (the library and the numpy judge each lie within the bound of the long-double run)
    XB, covB = S["B"][0], S["B"][1]
    dcs = b[0] + b[1]
    dp = dcs * np.abs(XB[:, :2]).sum(1).max() + b[2:].max()
    f_px = max(cfg["intrinsics"][:2]); z_min = float(rec2["depth"].min()); tr = float(np.trace(covB, axis1=1, axis2=2).max())
    d_px = 4 * f_px * dp / z_min
    d_rad = 3.0 / 2.0 * (f_px / z_min) ** 2 * (4 * dcs * tr + 2 * tr * dp / z_min)
    print("pushed through: dp %.3g m, d px %.3g, d radius %.3g, z_min %.1f m" % (dp, d_px, d_rad, z_min))
    sp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    for f, d in (("x", d_px), ("y", d_px), ("radius", d_rad)):
        assert np.all(np.abs(rec["q"][f].astype(np.float64) - rec2["q"][f]) <= d + sp(rec2["q"][f])), f
    assert np.all(np.abs(rec["depth"].astype(np.float64) - rec2["depth"]) <= dp + sp(rec2["depth"]))
    gpu.close()


def test_given_alignment_is_bit_for_bit(gpu_ctx, stream):
    frames, seq, cfg = stream
    S = C3.sessions()
    psi, t = S["truth"]
    fwd = ops.align_record((np.cos(-psi), np.sin(-psi), -(np.array([[np.cos(psi), np.sin(psi), 0], [-np.sin(psi), np.cos(psi), 0], [0, 0, 1.0]]) @ t)))[0]      # A -> B
    inv = ops.align_invert(fwd)
    ci, si, ti = L.invert_alignment(fwd)
    assert np.array([inv["c"], inv["s"], *inv["t"]]).tobytes() == np.array([ci, si, *ti]).tobytes()
    Q = np.random.default_rng(3).normal(size=(4, 4)); Pa = 1e-10 * (Q @ Q.T)      # (small against the points' own (1 cm)^2 even 40 m from the origin, so B's copies still win some)
    m = L.merge_maps(S["A"], S["B"], align=inv, cov_align=Pa, r_dup=P["r_dup"])
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    gpu.set_map(*S["A"])
    used, order, info, minfo = gpu.merge_map(*S["B"], align=inv, cov_align=Pa, r_dup=P["r_dup"])
    assert used.tobytes() == inv.tobytes() and not minfo.tobytes().strip(b"\0")
    assert order.tobytes() == m["order"].tobytes() and info.tobytes() == m["info"].tobytes() and gpu.map_size == len(order)
    assert int(info["n_duplicate"]) == P["n_shared"] and (order >= P["n_a"]).sum() > P["n_new"]           # some of B's copies won
    rec, minf = _match(gpu)
    gpu.set_map(m["X"], m["cov"], m["desc"])
    rec2, minf2 = _match(gpu)
    assert rec.tobytes() == rec2.tobytes() and minf.tobytes() == minf2.tobytes() and minf["n_selected"] >= 50
    gpu.close()


def test_no_overlap_is_an_answer_and_refusals_leave_the_map(gpu_ctx, stream):
    import larvio_amd
    from larvio_amd._lib import lib, _p, ALIGN_RESULT, MAP_BUILD_INFO, GLOBAL_INFO
    frames, seq, cfg = stream
    S = C3.sessions()
    XA, covA, dA = S["A"]; XB, covB, dB = (np.ascontiguousarray(a) for a in S["B"])
    gpu = _frontend(gpu_ctx, cfg)
    MC.drive(_step(gpu), frames, seq, 3)
    res = np.zeros(1, ALIGN_RESULT); out = np.zeros(1024, np.int32); bi = np.zeros(1, MAP_BUILD_INFO); gi = np.zeros(1, GLOBAL_INFO)
    covB9 = covB.reshape(-1, 9)

    def raw(h_X=XB, h_cov=covB9, h_desc=dB, n=len(XB), align=None, ao=None, bo=None, mo=None, mh=0, h_res=res, cap=1024):
        return lib().lvk_frontend_merge_map(gpu._h, _p(h_X), _p(h_cov), _p(h_desc), n, _p(align), None, C.byref(mo) if mo is not None else None,
                                            C.byref(ao) if ao is not None else None, mh, 7, C.byref(bo) if bo is not None else None, _p(h_res), _p(out), cap, _p(bi), _p(gi))
    assert raw() == 1                                                                    # no map is set
    gpu.set_map(XA, None, dA)
    assert raw() == 1 and gpu.map_size == P["n_a"]                                        # the resident map has no covariances
    gpu.set_map(XA, covA, dA)
    before = tuple(a.tobytes() for a in _match(gpu))
    # ---- no overlap: B's new points alone
    k = P["n_shared"]
    used, order, info, minfo = gpu.merge_map(XB[k:], covB[k:], dB[k:], r_dup=P["r_dup"])
    assert used["status"] == R3.NO_MODEL and len(order) == 0 and not info.tobytes().strip(b"\0") and minfo["n_selected"] == 0
    assert gpu.map_size == P["n_a"] and tuple(a.tobytes() for a in _match(gpu)) == before
    # ---- refusals
    O3, OB = ops.align3d_options, ops.map_build_options
    from larvio_amd._lib import MatchOptions
    bad = ops.align_record((np.nan, 0.0, np.zeros(3)))
    for code, kw in ((1, dict(h_cov=None)), (1, dict(h_desc=None)), (1, dict(h_X=None)), (1, dict(n=-1)), (1, dict(cap=-1)), (1, dict(mh=-1)), (1, dict(h_res=None)),
                     (1, dict(ao=O3(thresh=-1.0))), (1, dict(ao=O3(min_inliers=1))), (1, dict(bo=OB(r_dup=float("nan")))), (1, dict(bo=OB(dup_max_dist=300))),
                     (1, dict(mo=MatchOptions(0, 0.0, 0.0, 300, 0))), (1, dict(mo=MatchOptions(0, 0.0, 0.0, 0, 101))), (1, dict(align=bad)),
                     (3, dict(mh=4097)), (3, dict(n=(1 << 20) - P["n_a"] + 1)), (3, dict(cap=10))):
        assert raw(**kw) == code, kw
        assert lib().lvk_last_error(gpu_ctx.h)
        assert gpu.map_size == P["n_a"], kw
    assert tuple(a.tobytes() for a in _match(gpu)) == before                              # the map in force stayed
    with pytest.raises(larvio_amd.LvkError):
        gpu.merge_map(XB, covB, dB, thresh=-1.0)
    # with an alignment given the search does not run: its options are not read, a non-finite covariance of the alignment is refused
    ident = ops.align_record((1.0, 0.0, np.zeros(3)))
    badP = np.eye(4).reshape(16); badP[5] = np.inf
    assert lib().lvk_frontend_merge_map(gpu._h, _p(XB), _p(covB9), _p(dB), len(XB), _p(ident), _p(badP), None, None, 0, 7, None, _p(res), _p(out), 1024, _p(bi), _p(gi)) == 1
    assert b"cov_align16" in lib().lvk_last_error(gpu_ctx.h) and gpu.map_size == P["n_a"]
    # ---- the frame-boundary rule: between lvk_frontend_begin and the lvk_frontend_process of the same frame
    from larvio_amd._lib import make_image
    Lb = lib()
    Lb.lvk_frontend_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_double]; Lb.lvk_frontend_begin.restype = C.c_int
    ts, img = frames[3]
    im, keep = make_image(img)
    assert Lb.lvk_frontend_begin(gpu._h, C.byref(im), float(ts)) == 0
    out[:] = -7; res[:] = np.zeros(1, ALIGN_RESULT); res["status"] = -7
    assert raw() == 1 and b"still waiting for its lvk_frontend_process" in lib().lvk_last_error(gpu_ctx.h)
    assert raw(align=ident) == 1 and b"still waiting for its lvk_frontend_process" in lib().lvk_last_error(gpu_ctx.h)
    with pytest.raises(larvio_amd.LvkError, match="still waiting for its lvk_frontend_process"):
        gpu.merge_map(XB, covB, dB, r_dup=P["r_dup"])
    assert gpu.map_size == P["n_a"] and (out == -7).all() and res[0]["status"] == -7         # nothing of the caller's was written
    MC.drive(_step(gpu), frames[3:], seq, 1)                                                  # the frame's own process call: the handle goes on
    after = tuple(a.tobytes() for a in _match(gpu))
    gpu.set_map(XA, covA, dA)
    assert tuple(a.tobytes() for a in _match(gpu)) == after                                   # the map in force was A all along
    assert raw() == 0 and res[0]["status"] == R3.OK and gpu.map_size == bi[0]["n_kept"] == P["n_a"] + len(XB)      # and the handle goes on (no r_dup: nothing is a duplicate)
    MC.drive(_step(gpu), frames[4:], seq, 2)
    assert gpu.state == 3
    gpu.close()


def test_merges_between_frames_change_no_published_byte(gpu_ctx, stream):
    frames, seq, cfg = stream
    S = C3.sessions()
    plain = _frontend(gpu_ctx, cfg)
    want = MC.drive(_step(plain), frames, seq, 8)
    plain.close()
    gpu = _frontend(gpu_ctx, cfg)

    def after(i, img):
        if i == 2:
            gpu.set_map(*S["A"])
        if i in (3, 5):
            used, order, info, minfo = gpu.merge_map(*S["B"], r_dup=P["r_dup"], seed=7)
            assert used["status"] == R3.OK and gpu.map_size == P["n_a"] + P["n_new"]     # the second merge finds all of B in the map already
    got = MC.drive(_step(gpu), frames, seq, 8, after=after)
    assert got == want and any(want)
    gpu.close()
