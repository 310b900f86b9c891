"""GPU: the 3D-3D alignment's stage entry (lvk_align_ransac_3d) on every case of tests/align3d_cases.py against tests/align3d_ref.py.

bit for bit   every hypothesis record (n_models, count, c, s, t, the zero pads, all zero without a model), the winner's hypothesis and
              pair, the mask bytes, the status, the inlier count, the winner's c0, s0, t0 - against the float64 restatement, whose discrete
              results the CPU test shows to be the long-double judge's
inside bound  the refined c, s, t, A and rms against the long-double judge - the sums run across the lanes in another order than
              numpy's - inside align3d_ref.bounds (operation counts only).  The worst |error| / bound per group is printed
the same bits twice, with NaN in every match beyond n and junk in every pair beyond n_pairs, with and without the caller's record
buffer; the sentinel bytes around the records, the mask and the result untouched; every refusal followed by a good call."""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, ALIGN3D_HYP, ALIGN_RESULT
from tests import align3d_cases as C3
from tests import align3d_ref as R3

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3
WORST = {}


def _opt(k):
    return ops.align3d_options(**k["opt"])


def _run(ctx, k, pad=0, **kw):
    n, P = len(k["X"]), len(k["pairs"])
    return ops.align_ransac_3d(ctx, C3.match_records(k, pad), C3.pair_records(k, pad), _opt(k), n=n, n_pairs=P, **kw)


def _ratio(group, err, bound):
    err = np.abs(np.asarray(err, R3.LD)); bound = np.asarray(bound, R3.LD)
    err, bound = np.broadcast_arrays(err, bound)
    assert np.all(np.isfinite(err)), group
    with np.errstate(all="ignore"):
        r = float(np.max(np.where(err == 0, 0, np.where(bound > 0, err / bound, np.inf)), initial=0.0))      # an error where the bound is 0 is over it
    WORST[group] = max(WORST.get(group, 0.0), r)
    return r


def _guards_untouched(out):
    G = ops.ALIGN_GUARD
    for k in ("hyp_raw", "mask_raw", "result_raw"):
        assert (out[k][:G] == 0xA5).all() and (out[k][-G:] == 0xA5).all(), k


@pytest.mark.parametrize("name", list(C3.cases()))
def test_case_is_the_restatements(gpu_ctx, name):
    k = C3.cases()[name]
    ref = C3.reference(name); f64 = C3.reference(name, "f64"); bnd = C3.reference_bounds(name)
    out = _run(gpu_ctx, k)
    _guards_untouched(out)
    hyp, res, P = out["hyp"], out["result"], len(k["pairs"])
    if len(k["X"]) < 2:                                   # no pair is looked at: the records stay as they were
        assert (out["hyp_raw"] == 0xA5).all()
    else:
        assert np.array_equal(hyp["n_models"], f64["n_models"]), np.nonzero(hyp["n_models"] != f64["n_models"])[0][:8]
        assert np.array_equal(hyp["count"], f64["count"]) and not hyp["pad"].any()
        for fld in ("c", "s", "t"):
            assert hyp[fld].tobytes() == np.ascontiguousarray(f64[fld], np.float64).tobytes(), (name, fld)
        assert not np.ascontiguousarray(hyp).view(np.uint8).reshape(P, ALIGN3D_HYP.itemsize)[f64["n_models"] == 0].any()          # all zero without a model
    assert res["status"] == ref["status"] == k["want"].get("status", ref["status"])
    assert (res["hyp"], res["root"], res["n_inliers"], res["iters"], res["pad"]) == (ref["hyp"], 0 if ref["hyp"] >= 0 else -1, ref["n_inliers"], 0, 0)
    pi, pj = (k["pairs"][ref["hyp"]] if ref["hyp"] >= 0 else (-1, -1))
    assert (res["pair_i"], res["pair_j"]) == (pi, pj)
    assert np.array_equal(out["mask"], ref["mask"]) and int(out["mask"].sum()) == (ref["n_inliers"] if ref["hyp"] >= 0 else 0)
    got0 = np.array([res["c0"], res["s0"], *res["t0"]]); got = np.array([res["c"], res["s"], *res["t"]])
    if ref["hyp"] < 0:
        assert np.array_equal(got, [1, 0, 0, 0, 0]) and np.array_equal(got0, got) and not res["A"].any() and res["rms"] == 0
        return
    m0 = f64["min_model"]
    assert got0.tobytes() == np.array([m0[0], m0[1], *m0[2]], np.float64).tobytes()                              # the winner, bit for bit
    if ref["status"] == R3.FEW_INLIERS:
        assert got.tobytes() == got0.tobytes() and not res["A"].any() and res["rms"] == 0
        return
    want = np.array([ref["model"][0], ref["model"][1], *ref["model"][2]], R3.LD)
    if ref["status"] == R3.SINGULAR:
        assert got.tobytes() == got0.tobytes()                                                                   # the winner is returned
        r = [0.0]
    else:
        r = [_ratio("refined model", got.astype(R3.LD) - want, bnd["model"])]
    r += [_ratio("A", res["A"].astype(R3.LD) - ref["A"], bnd["A"]), _ratio("rms", R3.LD(res["rms"]) - ref["rms"], bnd["rms"])]
    print(name, "worst |error| / bound: refined model %.3f, A %.3f, rms %.3f" % tuple(r))
    assert max(r) <= 1.0, (name, r)
    assert abs(float(res["c"]) ** 2 + float(res["s"]) ** 2 - 1.0) <= 1e-14
    assert res["A"].tobytes() == res["A"].T.copy().tobytes() and res["A"][1, 1] == res["A"][2, 2] == res["A"][3, 3] == ref["n_inliers"]


def test_worst_ratios_are_reported():
    """(runs behind the cases: prints the worst ratios)"""
    print("worst |error| / bound per group:", {g: round(v, 4) for g, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


@pytest.mark.parametrize("name", ["n65_out60_all_pairs", "n1024_out80_4096", "n3_bad_indices_5", "vertical_line", "all_wrong"])
def test_same_bits_twice_and_with_junk_behind_the_counts(gpu_ctx, name):
    k = C3.cases()[name]
    a = _run(gpu_ctx, k); b = _run(gpu_ctx, k); c = _run(gpu_ctx, k, pad=7); d = _run(gpu_ctx, k, want_hyp=False)
    P = ALIGN3D_HYP.itemsize * len(k["pairs"]); n = len(k["X"]); G = ops.ALIGN_GUARD
    for o in (b, c):
        assert o["hyp"].tobytes()[:P] == a["hyp"].tobytes() and o["mask"].tobytes()[:n] == a["mask"].tobytes() and o["result"].tobytes() == a["result"].tobytes()
        _guards_untouched(o)
    assert d["mask"].tobytes() == a["mask"].tobytes() and d["result"].tobytes() == a["result"].tobytes()
    assert (d["hyp_raw"] == 0xA5).all()                   # without a record buffer nothing of the caller's is written
    # the fill behind n matches' mask bytes and n_pairs records stays: give the buffers room for more than the counts say
    m = C3.match_records(k, 7); pr = C3.pair_records(k, 7)
    o = ops.align_ransac_3d(gpu_ctx, m, pr, _opt(k), n=n, n_pairs=len(k["pairs"]))                # (sized by the counts: the guards are the fill)
    _guards_untouched(o)
    assert (o["mask_raw"][G + n:] == 0xA5).all() and (o["hyp_raw"][G + P:] == 0xA5).all()


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    k = C3.cases()["n64_out30_64"]
    good_out = _run(ctx, k)
    m = C3.match_records(k); pr = C3.pair_records(k)
    d_m = ctx.to_device(m.view(np.uint8)); d_pr = ctx.to_device(pr.view(np.uint8))
    fill_h = np.full(ALIGN3D_HYP.itemsize * 64, 0x5A, np.uint8); fill_m = np.full(64, 0x5A, np.uint8); fill_r = np.full(ALIGN_RESULT.itemsize, 0x5A, np.uint8)
    d_h = ctx.to_device(fill_h); d_mask = ctx.to_device(fill_m); d_r = ctx.to_device(fill_r)
    good = dict(d_m=d_m, n=64, d_pr=d_pr, n_pairs=64, opt=_opt(k), d_h=d_h, d_mask=d_mask, d_r=d_r)

    def raw(a):
        return lib().lvk_align_ransac_3d(ctx.h, _p(a["d_m"]), a["n"], _p(a["d_pr"]), a["n_pairs"], C.byref(a["opt"]) if a["opt"] is not None else None, _p(a["d_h"]),
                                         _p(a["d_mask"]), _p(a["d_r"]))

    def read():
        ctx.sync()
        return ctx.to_host(d_h, np.uint8, fill_h.shape).tobytes(), ctx.to_host(d_mask, np.uint8, (64,)).tobytes(), ctx.to_host(d_r, np.uint8, fill_r.shape).tobytes()

    def refill():
        for d, f in ((d_h, fill_h), (d_mask, fill_m), (d_r, fill_r)):
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(d.ptr), _p(f), f.nbytes))

    def refused(code, **ch):
        a = dict(good); a.update(ch)
        assert raw(a) == code, ch
        assert lib().lvk_last_error(ctx.h)
        assert read() == (fill_h.tobytes(), fill_m.tobytes(), fill_r.tobytes()), ch          # nothing was launched
        assert raw(good) == LVK_OK                                                           # the context goes on
        assert read() == (good_out["hyp"].tobytes(), good_out["mask"].tobytes(), good_out["result"].tobytes()), ch
        refill()

    O = ops.align3d_options
    for ch in (dict(d_m=None), dict(d_pr=None), dict(d_mask=None), dict(d_r=None), dict(n=-1), dict(n_pairs=-1), dict(opt=O(thresh=-0.1)), dict(opt=O(thresh=np.nan)),
               dict(opt=O(min_rho=np.inf)), dict(opt=O(min_rho=-0.5)), dict(opt=O(min_inliers=1)), dict(opt=O(min_inliers=1025))):
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n=1025)
    refused(LVK_ERR_CAPACITY, n_pairs=4097)
    # options left out altogether are the defaults; n < 2 and n_pairs == 0 are NO_MODEL with the mask zeroed and no record written
    a = dict(good); a["opt"] = None
    assert raw(a) == LVK_OK
    want = ops.align_ransac_3d(ctx, m, pr, O())
    assert read()[1:] == (want["mask"].tobytes(), want["result"].tobytes())
    for ch in (dict(n=1), dict(n_pairs=0, d_pr=None), dict(n=0, d_m=None, d_mask=None)):
        refill()
        a = dict(good); a.update(ch)
        assert raw(a) == LVK_OK, ch
        h, mk, r = read()
        res = np.frombuffer(r, ALIGN_RESULT)[0]
        assert h == fill_h.tobytes() and res["status"] == R3.NO_MODEL and res["hyp"] == -1 and res["c"] == 1.0, ch
        nn = a["n"]
        assert mk == bytes(nn) + fill_m.tobytes()[nn:], ch
