"""GPU: the prior-map selection's stage entry (lvk_map_select_queries) on every case of tests/map_select_cases.py.

exact        status bytes (bit 7 included), d_info, the selected indices in their order, cell, depth and the gathered descriptors equal
             the numpy restatement (tests/map_select_ref.py) byte for byte; the query records repeat the selection records; records beyond
             n_selected and the sentinel bytes around every buffer are untouched
float32      x, y and radius are equal or adjacent float32 values to the long-double judge's (a correctly rounded FP64 chain can differ from
             it only at a rounding midpoint); how many were not equal is printed (PARITY.md quotes it)
the same bytes twice on the 70,000-point case; without descriptors and without a status buffer; every refusal followed by a good call."""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, MAP_SEL, MAP_INFO, MATCH_QUERY, ALIGN_RESULT
from tests import map_select_cases as MC
from tests import map_select_ref as R

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3
NOT_EQUAL = {"x": 0, "y": 0, "radius": 0, "n": 0}


def _run(ctx, k, **kw):
    return ops.map_select_queries(ctx, k["X"], k["cov"], k["desc"], k["cam"], k["R_wc"], k["p_wc"], align=k["align"], cov_cam=k["cov_cam"],
                                  options=ops.map_select_options(**k["opt"]), **kw)


def _guards_untouched(out, n_sel):
    G = ops.MAP_GUARD
    for f in ("sel_raw", "q_raw", "q_desc_raw", "info_raw", "status_raw"):
        assert (out[f][:G] == 0xA5).all() and (out[f][-G:] == 0xA5).all(), f
    for f, size in (("sel_raw", MAP_SEL.itemsize), ("q_raw", MATCH_QUERY.itemsize), ("q_desc_raw", 32)):
        assert (out[f][G + size * n_sel:] == 0xA5).all(), f          # nothing behind the last record


@pytest.mark.parametrize("name", list(MC.cases()))
def test_case_is_the_restatements(gpu_ctx, name):
    k = MC.cases()[name]; ref = MC.reference(name); j = MC.judged(name)
    out = _run(gpu_ctx, k)
    n_sel = int(ref["info"]["n_selected"])
    assert out["info"].tobytes() == ref["info"].tobytes(), (out["info"], ref["info"])
    assert out["status"].tobytes() == ref["status"].tobytes(), np.nonzero(out["status"] != ref["status"])[0][:8]
    _guards_untouched(out, n_sel)
    sel = out["sel"]
    for f in ("index", "cell", "depth"):
        assert sel[f].tobytes() == ref["sel"][f].tobytes(), (f, sel[f][:8], ref["sel"][f][:8])
    assert out["q_desc"].tobytes() == ref["q_desc"].tobytes()
    for f in ("x", "y", "radius"):
        assert out["q"][f].tobytes() == sel[f].tobytes()
        want = j[f][ref["sel"]["index"]]
        assert R.adjacent_or_equal(sel[f], want).all(), (f, sel[f][~R.adjacent_or_equal(sel[f], want)][:4])
        NOT_EQUAL[f] += int((sel[f] != want).sum())
    NOT_EQUAL["n"] += n_sel
    assert not out["q"]["pad"].any()
    if "last_radius" in k["want"]:
        assert sel["radius"][sel["index"] == len(k["X"]) - 1] == np.float32(k["want"]["last_radius"])


def test_not_equal_counts_are_reported():
    """(runs behind the cases: prints what PARITY.md quotes)"""
    print("float32 values not equal to the long-double judge's (all adjacent):", NOT_EQUAL)
    assert all(NOT_EQUAL[f] <= NOT_EQUAL["n"] for f in ("x", "y", "radius"))


def test_same_bytes_twice_on_the_large_case(gpu_ctx):
    k = MC.cases()["n70000_radtan_cov_cc_align"]
    a = _run(gpu_ctx, k); b = _run(gpu_ctx, k)
    for f in ("sel_raw", "q_raw", "q_desc_raw", "info_raw", "status_raw"):
        assert a[f].tobytes() == b[f].tobytes(), f


def test_without_descriptors_and_without_a_status_buffer(gpu_ctx):
    k = dict(MC.cases()["n5000_radtan_cov_cc_align"]); ref = MC.reference("n5000_radtan_cov_cc_align")
    full = _run(gpu_ctx, k)
    k["desc"] = None
    out = _run(gpu_ctx, k, want_status=False)
    assert out["sel"].tobytes() == full["sel"].tobytes() and out["info"].tobytes() == ref["info"].tobytes()
    assert (out["q_desc_raw"] == 0xA5).all() and (out["status_raw"] == 0xA5).all()


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    k = MC.cases()["n257_radtan_cc"]; ref = MC.reference("n257_radtan_cc")
    n = len(k["X"])
    d_X = ctx.to_device(k["X"]); d_cov = ctx.to_device(np.tile(1e-4 * np.eye(3).reshape(9), (n, 1))); d_desc = ctx.to_device(k["desc"])
    fill = {f: np.full(size, 0x5A, np.uint8) for f, size in (("sel", MAP_SEL.itemsize * 1024), ("q", MATCH_QUERY.itemsize * 1024), ("qd", 32 * 1024 + 8), ("info", MAP_INFO.itemsize),
                                                           ("st", n))}
    dev = {f: ctx.to_device(v) for f, v in fill.items()}
    R9 = np.ascontiguousarray(k["R_wc"], np.float64).reshape(9); p3 = np.ascontiguousarray(k["p_wc"], np.float64); cc = np.ascontiguousarray(k["cov_cam"]).reshape(36)
    good = dict(d_X=d_X, d_cov=None, d_desc=d_desc, n=n, cam=ops.map_camera(k["cam"]), align=None, R=R9, p=p3, cc=cc, opt=ops.map_select_options(), sel=dev["sel"], q=dev["q"],
                qd=dev["qd"], info=dev["info"], st=dev["st"])

    def raw(a):
        return lib().lvk_map_select_queries(ctx.h, _p(a["d_X"]), _p(a["d_cov"]), _p(a["d_desc"]), a["n"], C.byref(a["cam"]) if a["cam"] is not None else None, _p(a["align"]),
                                            _p(a["R"]), _p(a["p"]), _p(a["cc"]), C.byref(a["opt"]) if a["opt"] is not None else None, _p(a["sel"]), _p(a["q"]), _p(a["qd"]),
                                            _p(a["info"]), _p(a["st"]))

    def read():
        ctx.sync()
        return {f: ctx.to_host(dev[f], np.uint8, fill[f].shape).tobytes() for f in fill}

    def refill():
        for f in fill:
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(dev[f].ptr), _p(fill[f]), fill[f].nbytes))

    def is_good(got):
        ns = int(ref["info"]["n_selected"])
        assert got["info"] == ref["info"].tobytes() and got["st"] == ref["status"].tobytes()
        assert got["sel"][:MAP_SEL.itemsize * ns] == ref["sel"].tobytes() and got["qd"][:32 * ns] == ref["q_desc"].tobytes()

    def refused(code, **ch):
        a = dict(good); a.update(ch)
        assert raw(a) == code, ch
        assert lib().lvk_last_error(ctx.h)
        assert read() == {f: v.tobytes() for f, v in fill.items()}, ch                      # nothing was launched
        assert raw(good) == LVK_OK                                                          # the context goes on
        is_good(read())
        refill()

    def cam(**ch):
        c = dict(k["cam"]); c.update(ch)
        return ops.map_camera(c)

    bad_R = R9.copy(); bad_R[4] = np.nan
    bad_p = p3.copy(); bad_p[2] = np.inf
    bad_align = np.zeros(1, ALIGN_RESULT); bad_align["c"] = 1.0; bad_align["t"][0, 1] = np.nan
    O = ops.map_select_options
    for ch in (dict(d_X=None), dict(cam=None), dict(R=None), dict(p=None), dict(sel=None), dict(q=None), dict(qd=None), dict(info=None), dict(n=-1), dict(R=bad_R), dict(p=bad_p),
               dict(align=bad_align), dict(cam=cam(intrinsics=(np.nan, 457.0, 367.0, 248.0))), dict(cam=cam(distortion=(0.0, np.inf, 0.0, 0.0))), dict(cam=cam(distortion_model=2)),
               dict(cam=cam(width=0)), dict(opt=O(r_min=50.0)), dict(opt=O(r_min=10.0, r_max=5.0)), dict(opt=O(rows=17)), dict(opt=O(cols=-1)), dict(opt=O(cols=17)), dict(opt=O(quota=-1)),
               dict(opt=O(rows=4, cols=5, quota=52)), dict(opt=O(rows=16, cols=16, quota=5)), dict(opt=O(quota=1025, rows=1, cols=1)), dict(opt=O(margin=-1.0)), dict(opt=O(k_sigma=np.nan)),
               dict(d_desc=d_desc.ptr + 4), dict(qd=dev["qd"].ptr + 4)):
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n=(1 << 20) + 1)
    # options left out are the defaults; a covariance pointer changes the radii only; n == 0 zeroes d_info and writes nothing else
    a = dict(good); a["opt"] = None
    assert raw(a) == LVK_OK
    is_good(read())
    a = dict(good); a["d_cov"] = d_cov
    assert raw(a) == LVK_OK
    got = read()
    ns = int(ref["info"]["n_selected"])
    sel = np.frombuffer(got["sel"], MAP_SEL)[:ns]
    assert got["info"] == ref["info"].tobytes() and np.array_equal(sel["index"], ref["sel"]["index"]) and (sel["radius"] >= ref["sel"]["radius"]).all()
    refill()
    for ch in (dict(n=0), dict(n=0, d_X=None, sel=None, q=None, qd=None, d_desc=None, st=None)):
        a = dict(good); a.update(ch)
        assert raw(a) == LVK_OK, ch
        got = read()
        assert got["info"] == bytes(MAP_INFO.itemsize) and all(got[f] == fill[f].tobytes() for f in ("sel", "q", "qd", "st")), ch
        refill()
