"""GPU: the map build's stage entry (lvk_map_build) on every case of tests/map_build_cases.py.

exact        d_order, the three gathered arrays, d_status and d_info equal the numpy restatement (tests/map_build_ref.py) byte for byte; the
             bytes beyond n_kept in every output buffer and the sentinel bytes around them are untouched; the case's planted property holds
first call   the same as the first call of a fresh context, and twice in a row on one context (the work buffers are reused)
refusals     every LVK_ERR_ARG / LVK_ERR_CAPACITY condition returns its code and launches nothing; the context serves a good call afterwards
null inputs  an output buffer whose input is NULL - preallocated outputs reused for a map without covariances or descriptors - keeps its fill"""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, MAP_BUILD_INFO
from tests import map_build_cases as MC

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3
RECORD = dict(order=4, X=24, cov=72, desc=32)


def _run(ctx, k, **kw):
    return ops.map_build(ctx, k["X"], k["cov"], k["desc"], k["score"], ops.map_build_options(**k["opt"]), **kw)


def _is_the_reference(out, ref, k):
    n = len(k["X"]); nk = int(ref["info"]["n_kept"]); G = ops.MAP_BUILD_GUARD
    assert out["info"].tobytes() == ref["info"].tobytes(), (out["info"], ref["info"])
    assert out["status"].tobytes() == ref["status"].tobytes(), np.nonzero(out["status"] != ref["status"])[0][:8]
    assert out["order"].tobytes() == ref["order"].tobytes(), (out["order"][:8], ref["order"][:8])
    assert out["X"].tobytes() == ref["X"].tobytes()
    for f in ("cov", "desc"):
        assert (out[f] is None) == (ref[f] is None) and (ref[f] is None or out[f].tobytes() == ref[f].tobytes()), f
    for f, size in RECORD.items():
        raw = out[f + "_raw"]
        assert (raw[:G] == 0xA5).all() and (raw[-G:] == 0xA5).all(), f
        if k[f if f in ("cov", "desc") else "X"] is None:
            assert (raw == 0xA5).all(), f
        else:
            assert len(raw) == 2 * G + size * n and (raw[G + size * nk:] == 0xA5).all(), f       # nothing behind the last kept record
    for f in ("status_raw", "info_raw"):
        assert (out[f][:G] == 0xA5).all() and (out[f][-G:] == 0xA5).all(), f


@pytest.mark.parametrize("name", MC.NAMES)
def test_case_is_the_restatements(gpu_ctx, name):
    k = MC.case(name); ref = MC.reference(name)
    out = _run(gpu_ctx, k)
    _is_the_reference(out, ref, k)
    MC.check_want(name, out["status"], out["order"])


@pytest.mark.parametrize("name", ["n257", "n3000", "crowd_300"])
def test_first_call_of_a_fresh_context_and_twice_in_a_row(name):
    import larvio_amd
    k = MC.case(name); ref = MC.reference(name)
    ctx = larvio_amd.Context(0)
    try:
        a = _run(ctx, k)
        _is_the_reference(a, ref, k)
        b = _run(ctx, k)                                                     # the work buffer of the first call, reused
        for f in a:
            if f.endswith("_raw"):
                assert a[f].tobytes() == b[f].tobytes(), f
        small = MC.case("n65")                                               # a smaller call in the larger call's buffer, then the larger one again
        _is_the_reference(_run(ctx, small), MC.reference("n65"), small)
        _is_the_reference(_run(ctx, k), ref, k)
    finally:
        ctx.close()


def test_without_a_status_buffer_and_without_descriptors(gpu_ctx):
    k = dict(MC.case("n1000_nodedup")); ref = MC.reference("n1000_nodedup")
    out = _run(gpu_ctx, k, want_status=False)
    assert out["order"].tobytes() == ref["order"].tobytes() and out["info"].tobytes() == ref["info"].tobytes() and (out["status_raw"] == 0xA5).all()
    k["desc"] = None                                                         # allowed while de-duplication is off
    out = _run(gpu_ctx, k)
    assert out["order"].tobytes() == ref["order"].tobytes() and out["status"].tobytes() == ref["status"].tobytes() and (out["desc_raw"] == 0xA5).all()


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    k = MC.case("n257"); ref = MC.reference("n257")
    n = len(k["X"]); nk = int(ref["info"]["n_kept"])
    d_X = ctx.to_device(k["X"]); d_cov = ctx.to_device(k["cov"]); d_desc = ctx.to_device(np.concatenate([k["desc"].reshape(-1), np.zeros(8, np.uint8)]))
    fill = {f: np.full(size, 0x5A, np.uint8) for f, size in (("order", 4 * n), ("X", 24 * n), ("cov", 72 * n), ("desc", 32 * n + 8), ("st", n), ("info", MAP_BUILD_INFO.itemsize))}
    dev = {f: ctx.to_device(v) for f, v in fill.items()}
    O = ops.map_build_options
    good = dict(d_X=d_X, d_cov=d_cov, d_desc=d_desc, d_score=None, n=n, opt=O(**k["opt"]), order=dev["order"], X=dev["X"], cov=dev["cov"], desc=dev["desc"], st=dev["st"],
                info=dev["info"])

    def raw(a):
        return lib().lvk_map_build(ctx.h, _p(a["d_X"]), _p(a["d_cov"]), _p(a["d_desc"]), _p(a["d_score"]), a["n"], C.byref(a["opt"]) if a["opt"] is not None else None,
                                   _p(a["order"]), _p(a["X"]), _p(a["cov"]), _p(a["desc"]), _p(a["st"]), _p(a["info"]))

    def read():
        ctx.sync()
        return {f: ctx.to_host(dev[f], np.uint8, fill[f].shape).tobytes() for f in fill}

    def refill():
        for f in fill:
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(dev[f].ptr), _p(fill[f]), fill[f].nbytes))

    def is_good(got):
        assert got["info"] == ref["info"].tobytes() and got["st"] == ref["status"].tobytes()
        assert got["order"][:4 * nk] == ref["order"].tobytes() and got["X"][:24 * nk] == ref["X"].tobytes()
        assert got["cov"][:72 * nk] == ref["cov"].tobytes() and got["desc"][:32 * nk] == ref["desc"].tobytes()

    def refused(code, **ch):
        a = dict(good); a.update(ch)
        assert raw(a) == code, ch
        assert lib().lvk_last_error(ctx.h)
        assert read() == {f: v.tobytes() for f, v in fill.items()}, ch                      # nothing was launched
        assert raw(good) == LVK_OK                                                          # the context goes on
        is_good(read())
        refill()

    for ch in (dict(d_X=None), dict(order=None), dict(X=None), dict(cov=None), dict(desc=None), dict(info=None), dict(n=-1), dict(opt=O(max_score=np.nan)),
               dict(opt=O(r_dup=np.nan)), dict(opt=O(max_score=-1.0)), dict(opt=O(r_dup=-0.5)), dict(opt=O(r_dup=0.25, dup_max_dist=257)), dict(opt=O(dup_max_dist=-1)),
               dict(d_desc=d_desc.ptr + 4), dict(desc=dev["desc"].ptr + 4), dict(d_desc=None, desc=None)):              # the last: r_dup > 0 without descriptors
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n=(1 << 20) + 1)
    # n == 0 zeroes d_info and writes nothing else, with or without the other pointers
    for ch in (dict(n=0), dict(n=0, d_X=None, d_cov=None, d_desc=None, order=None, X=None, cov=None, desc=None, st=None)):
        a = dict(good); a.update(ch)
        assert raw(a) == LVK_OK, ch
        got = read()
        assert got["info"] == bytes(MAP_BUILD_INFO.itemsize) and all(got[f] == fill[f].tobytes() for f in ("order", "X", "cov", "desc", "st")), ch
        refill()
    # options left out are the defaults: no de-duplication, nothing uncertain
    a = dict(good); a["opt"] = None
    assert raw(a) == LVK_OK
    from tests import map_build_ref as R
    want = R.build(k["X"], k["cov"], k["desc"], None)
    got = read()
    assert got["info"] == want["info"].tobytes() and got["order"][:4 * len(want["order"])] == want["order"].tobytes() and got["st"] == want["status"].tobytes()
    refill()
    # an output buffer whose input is NULL (preallocated outputs reused for a map without covariances or descriptors) is not touched, and
    # its alignment is nobody's business
    sc = np.linspace(0.008, 0.001, n)                                                     # under the case's max_score, the best last
    d_score = ctx.to_device(sc)
    for ch, inputs in ((dict(d_cov=None, d_score=d_score), (None, k["desc"])), (dict(d_desc=None, d_score=d_score, opt=O()), (k["cov"], None)),
                       (dict(d_cov=None, d_desc=None, desc=dev["desc"].ptr + 4, opt=None), (None, None))):
        a = dict(good); a.update(ch)
        assert raw(a) == LVK_OK, ch
        want = R.build(k["X"], inputs[0], inputs[1], sc if "d_score" in ch else None, **({} if a["opt"] is None or "opt" in ch else k["opt"]))
        got = read(); nw = len(want["order"])
        assert got["info"] == want["info"].tobytes() and got["order"][:4 * nw] == want["order"].tobytes() and got["X"][:24 * nw] == want["X"].tobytes(), ch
        for f, given in (("cov", inputs[0]), ("desc", inputs[1])):
            if given is None:
                assert got[f] == fill[f].tobytes(), (ch, f)                                 # the fill, every byte
            else:
                size = RECORD[f]
                assert got[f][:size * nw] == want[f].tobytes() and got[f][size * nw:] == fill[f].tobytes()[size * nw:], (ch, f)
        refill()
