"""GPU: the two-point alignment's stage entry (lvk_align_ransac_2pt) on every case of tests/align_cases.py against the long-double
restatement tests/align_ref.py.

exact        n_models, both counts and roots of every hypothesis, the winner's hypothesis, pair and root, the mask bytes, the status, the
             inlier count, the iterations, the zeros of the unused slots and pads
continuous   every model's c, s, t; the refined model, A and the rms - inside the restatement's first-order running error bound, doubled
             (align_ref.bounds: operation counts only).  The worst |error| / bound per group is printed (PARITY.md quotes it)
the same bits twice, with NaN in every match beyond n and junk in every pair beyond n_pairs, with and without the caller's record
buffer; the sentinel bytes around the records, the mask and the result untouched; every refusal followed by a good call."""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, ALIGN_HYP, ALIGN_RESULT
from tests import align_cases as AC
from tests import align_ref as AR

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3
WORST = {}


def _opt(k):
    return ops.align_options(**k["opt"])


def _run(ctx, k, pad=0, **kw):
    n, P = len(k["X"]), len(k["pairs"])
    return ops.align_ransac_2pt(ctx, AC.match_records(k, pad), AC.pair_records(k, pad), k["R_wc"], k["p_wc"], _opt(k), n=n, n_pairs=P, **kw)


def _ratio(group, err, bound):
    err = np.abs(np.asarray(err, AR.LD)); bound = np.asarray(bound, AR.LD)
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


@pytest.mark.parametrize("name", list(AC.cases()))
def test_case_is_the_restatements(gpu_ctx, name):
    k = AC.cases()[name]
    ref = AC.reference(name); bnd = AC.reference_bounds(name)
    out = _run(gpu_ctx, k)
    _guards_untouched(out)
    hyp, res, P = out["hyp"], out["result"], len(k["pairs"])
    if len(k["X"]) < 2:                                   # no pair is looked at: the records stay as they were
        assert (out["hyp_raw"] == 0xA5).all()
    else:
        assert np.array_equal(hyp["n_models"], ref["n_models"]), np.nonzero(hyp["n_models"] != ref["n_models"])[0][:8]
        assert (hyp["pad"] == 0).all()
        used = np.arange(2)[None, :] < ref["n_models"][:, None]
        assert np.array_equal(np.where(used, hyp["m"]["count"], -1), ref["count"])
        assert np.array_equal(np.where(used, hyp["m"]["root"], -1), ref["root"])
        assert not np.ascontiguousarray(hyp["m"]).view(np.uint8).reshape(P, 2, 48)[~used].any()      # slots beyond n_models are zero
        ratios = [_ratio("model " + f, (hyp["m"][f].astype(AR.LD) - ref[f])[used], bnd[f][used]) for f in ("c", "s", "t")] if used.any() else [0.0]
        assert max(ratios) <= 1.0, (name, ratios)
    assert res["status"] == ref["status"] == k["want"].get("status", ref["status"])
    assert (res["hyp"], res["root"], res["n_inliers"], res["iters"], res["pad"]) == (ref["hyp"], ref["root_w"], ref["n_inliers"], ref["iters"], 0)
    pi, pj = (k["pairs"][ref["hyp"]] if ref["hyp"] >= 0 else (-1, -1))
    assert (res["pair_i"], res["pair_j"]) == (pi, pj)
    assert np.array_equal(out["mask"], ref["mask"]) and int(out["mask"].sum()) == (ref["n_inliers"] if ref["hyp"] >= 0 else 0)
    got0 = np.array([res["c0"], res["s0"], *res["t0"]], AR.LD); want0 = np.array([ref["min_model"][0], ref["min_model"][1], *ref["min_model"][2]], AR.LD)
    got = np.array([res["c"], res["s"], *res["t"]], AR.LD); want = np.array([ref["model"][0], ref["model"][1], *ref["model"][2]], AR.LD)
    if ref["hyp"] < 0:
        assert np.array_equal(got, [1, 0, 0, 0, 0]) and np.array_equal(got0, got) and not res["A"].any() and res["rms"] == 0
        return
    w, ws = ref["hyp"], ref["slot"]
    assert got0.astype(np.float64).tobytes() == np.array([hyp["m"][w, ws]["c"], hyp["m"][w, ws]["s"], *hyp["m"][w, ws]["t"]]).tobytes()   # the winner's record, bit for bit
    r = [_ratio("refined model", got - want, bnd["model"]), _ratio("A", res["A"].astype(AR.LD) - ref["A"], bnd["A"] if ref["status"] != AR.FEW_INLIERS else np.ones((4, 4))),
         _ratio("rms", res["rms"] - ref["rms"], bnd["rms"] if ref["status"] != AR.FEW_INLIERS else 1.0)]
    print(name, "worst |error| / bound: refined model %.3f, A %.3f, rms %.3f" % tuple(r))
    assert max(r) <= 1.0, (name, r)
    if ref["status"] != AR.OK:
        assert got.tobytes() == got0.tobytes()                                      # the minimal model is returned as the refined one
    assert abs(float(res["c"]) ** 2 + float(res["s"]) ** 2 - 1.0) <= 1e-14


def test_worst_ratios_are_reported():
    """(runs behind the cases: prints what PARITY.md quotes)"""
    print("worst |error| / bound per group:", {g: round(v, 4) for g, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


@pytest.mark.parametrize("name", ["n65_out70_all_pairs", "n1024_out30_5", "n3_bad_indices_5", "rank_deficient"])
def test_same_bits_twice_and_with_junk_behind_the_counts(gpu_ctx, name):
    k = AC.cases()[name]
    a = _run(gpu_ctx, k); b = _run(gpu_ctx, k); c = _run(gpu_ctx, k, pad=7); d = _run(gpu_ctx, k, want_hyp=False)
    for o in (b, c):
        assert o["hyp"].tobytes() == a["hyp"].tobytes() and o["mask"].tobytes() == a["mask"].tobytes() and o["result"].tobytes() == a["result"].tobytes()
        _guards_untouched(o)
    assert d["mask"].tobytes() == a["mask"].tobytes() and d["result"].tobytes() == a["result"].tobytes()
    assert (d["hyp_raw"] == 0xA5).all()                   # without a record buffer nothing of the caller's is written


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    k = AC.cases()["n64_out30_4"]
    good_out = _run(ctx, k)
    m = AC.match_records(k); pr = AC.pair_records(k)
    R = np.ascontiguousarray(k["R_wc"], np.float64).reshape(9); p = np.ascontiguousarray(k["p_wc"], np.float64)
    d_m = ctx.to_device(m.view(np.uint8)); d_pr = ctx.to_device(pr.view(np.uint8))
    fill_h = np.full(ALIGN_HYP.itemsize * 4, 0x5A, np.uint8); fill_m = np.full(64, 0x5A, np.uint8); fill_r = np.full(ALIGN_RESULT.itemsize, 0x5A, np.uint8)
    d_h = ctx.to_device(fill_h); d_mask = ctx.to_device(fill_m); d_r = ctx.to_device(fill_r)
    good = dict(d_m=d_m, n=64, d_pr=d_pr, n_pairs=4, R=R, p=p, opt=_opt(k), d_h=d_h, d_mask=d_mask, d_r=d_r)

    def raw(a):
        return lib().lvk_align_ransac_2pt(ctx.h, _p(a["d_m"]), a["n"], _p(a["d_pr"]), a["n_pairs"], _p(a["R"]), _p(a["p"]), C.byref(a["opt"]) if a["opt"] is not None else None,
                                          _p(a["d_h"]), _p(a["d_mask"]), _p(a["d_r"]))

    def read():
        ctx.sync()
        return ctx.to_host(d_h, np.uint8, fill_h.shape).tobytes(), ctx.to_host(d_mask, np.uint8, (64,)).tobytes(), ctx.to_host(d_r, np.uint8, fill_r.shape).tobytes()

    def refused(code, **ch):
        a = dict(good); a.update(ch)
        assert raw(a) == code, ch
        assert lib().lvk_last_error(ctx.h)
        assert read() == (fill_h.tobytes(), fill_m.tobytes(), fill_r.tobytes()), ch          # nothing was launched
        assert raw(good) == LVK_OK                                                           # the context goes on
        assert read() == (good_out["hyp"].tobytes(), good_out["mask"].tobytes(), good_out["result"].tobytes()), ch
        for d, f in ((d_h, fill_h), (d_mask, fill_m), (d_r, fill_r)):
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(d.ptr), _p(f), f.nbytes))

    bad_R = R.copy(); bad_R[4] = np.nan
    bad_p = p.copy(); bad_p[2] = np.inf
    for ch in (dict(d_m=None), dict(d_pr=None), dict(d_mask=None), dict(d_r=None), dict(R=None), dict(p=None), dict(n=-1), dict(n_pairs=-1), dict(R=bad_R), dict(p=bad_p),
               dict(opt=ops.align_options(thresh=-0.01)), dict(opt=ops.align_options(thresh=np.nan)), dict(opt=ops.align_options(min_depth=np.inf)),
               dict(opt=ops.align_options(min_dz=-1e-6)), dict(opt=ops.align_options(min_inliers=1)), dict(opt=ops.align_options(min_inliers=1025)),
               dict(opt=ops.align_options(max_refine_iters=-1)), dict(opt=ops.align_options(max_refine_iters=101))):
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n=1025)
    refused(LVK_ERR_CAPACITY, n_pairs=4097)
    # options left out altogether are the defaults; n < 2 and n_pairs == 0 are NO_MODEL with the mask zeroed and no record written
    a = dict(good); a["opt"] = None
    assert raw(a) == LVK_OK
    want = ops.align_ransac_2pt(ctx, m, pr, k["R_wc"], k["p_wc"], ops.align_options())
    assert read()[1:] == (want["mask"].tobytes(), want["result"].tobytes())
    for ch in (dict(n=1), dict(n_pairs=0, d_pr=None), dict(n=0, d_m=None, d_mask=None)):
        for d, f in ((d_h, fill_h), (d_mask, fill_m), (d_r, fill_r)):
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(d.ptr), _p(f), f.nbytes))
        a = dict(good); a.update(ch)
        assert raw(a) == LVK_OK, ch
        h, mk, r = read()
        res = np.frombuffer(r, ALIGN_RESULT)[0]
        assert h == fill_h.tobytes() and res["status"] == AR.NO_MODEL and res["hyp"] == -1 and res["c"] == 1.0, ch
        nn = a["n"]
        assert mk == bytes(nn) + fill_m.tobytes()[nn:], ch
