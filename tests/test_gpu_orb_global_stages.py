"""GPU: the global ORB search's stage entry (lvk_orb_match_global) on every case of tests/orb_global_cases.py - best, the first n_selected
selection records and the counts must be the restatement's (tests/orb_global_ref.py, held to a brute-force loop by
tests/test_orb_global_ref.py), field for field and byte for byte, pads included; what lies beyond n_selected and around the buffers keeps
its 0x5A fill - and its refusals, each followed by a good call on the same context."""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, MATCH_RESULT, GLOBAL_MATCH, GLOBAL_INFO
from tests import orb_global_cases as GC
from tests import orb_global_ref as R

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3


def _run(ctx, k):
    return ops.orb_match_global(ctx, k["map_desc"], k["cand_desc"], k["max_dist"], k["ratio_pct"], k["max_matches"])


def _equal(name, got, want):
    for f in R.RESULT.names:
        assert np.array_equal(got["best"][f], want["best"][f]), (name, f, np.nonzero(got["best"][f] != want["best"][f])[0][:8])
    assert got["best"].tobytes() == want["best"].tobytes()
    assert got["info"].tobytes() == want["info"].tobytes(), (name, got["info"], want["info"])
    for f in R.GLOBAL_MATCH.names:
        assert np.array_equal(got["sel"][f], want["sel"][f]), (name, f)
    assert got["sel"].tobytes() == want["sel"].tobytes()
    G = ops.ORB_GLOBAL_GUARD
    ns = len(want["sel"]) * GLOBAL_MATCH.itemsize
    assert (got["sel_raw"][G + ns:] == 0x5A).all() and (got["sel_raw"][:G] == 0x5A).all(), name          # beyond n_selected: not touched
    for f in ("best_raw", "info_raw"):
        assert (got[f][:G] == 0x5A).all() and (got[f][-G:] == 0x5A).all(), (name, f)


@pytest.mark.parametrize("name", list(GC.cases()))
def test_case_equals_the_restatement(gpu_ctx, name):
    got = _run(gpu_ctx, GC.cases()[name])
    _equal(name, got, GC.reference(name))
    GC.check_want(name, got)


@pytest.mark.parametrize("name", ["n_map_0", "max_dist_edge", "pile_up_64"])
def test_first_call_on_a_fresh_context(name):
    """nothing may hang on what an earlier call left in the context: an empty map (no work buffer at all), a two-point map and the pile-up,
    each as the first call of a context of its own"""
    import larvio_amd
    ctx = larvio_amd.Context(0)
    try:
        got = _run(ctx, GC.cases()[name])
        _equal(name, got, GC.reference(name))
        GC.check_want(name, got)
    finally:
        ctx.close()


def test_a_second_call_starts_from_clean_claims(gpu_ctx):
    """the claim words live in the context's scratch: a pile-up must not leak into the next call, nor a larger map's table into a smaller one's"""
    _run(gpu_ctx, GC.cases()["pile_up_64"])
    for name in (f"random_m{GC.S + 1}_c65", "pile_up_64", "more_ok_than_max_matches", f"random_m{GC.S + 1}_c{GC.T + 1}"):
        _equal(name, _run(gpu_ctx, GC.cases()[name]), GC.reference(name))


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    name = "random_m65_c%d" % (GC.T + 1)
    k = GC.cases()[name]; want = GC.reference(name)
    nm, nc = len(k["map_desc"]), len(k["cand_desc"])
    fill = {"best": np.full(MATCH_RESULT.itemsize * nc, 0x5A, np.uint8), "sel": np.full(GLOBAL_MATCH.itemsize * 1024, 0x5A, np.uint8),
            "info": np.full(GLOBAL_INFO.itemsize, 0x5A, np.uint8)}
    d = {f: ctx.to_device(v) for f, v in fill.items()}
    d_md = ctx.to_device(np.concatenate([k["map_desc"].ravel(), np.zeros(8, np.uint8)]))
    d_cd = ctx.to_device(np.concatenate([k["cand_desc"].ravel(), np.zeros(8, np.uint8)]))
    names = ("d_md", "n_map", "d_cd", "n_cand", "max_dist", "ratio_pct", "max_matches", "d_best", "d_sel", "d_info")
    good = (d_md, nm, d_cd, nc, 58, 100, 1024, d["best"], d["sel"], d["info"])

    def raw(*a):
        return lib().lvk_orb_match_global(ctx.h, _p(a[0]), a[1], _p(a[2]), a[3], a[4], a[5], a[6], _p(a[7]), _p(a[8]), _p(a[9]))

    def read():
        ctx.sync()
        return {f: ctx.to_host(d[f], np.uint8, (len(fill[f]),)) for f in fill}

    def untouched(ch):
        got = read()
        assert all(got[f].tobytes() == fill[f].tobytes() for f in fill), ch

    def is_the_reference(ch):
        got = read()
        assert got["best"].tobytes() == want["best"].tobytes() and got["info"].tobytes() == want["info"].tobytes(), ch
        ns = len(want["sel"]) * GLOBAL_MATCH.itemsize
        assert got["sel"][:ns].tobytes() == want["sel"].tobytes() and (got["sel"][ns:] == 0x5A).all(), ch
        for f in fill:
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(d[f].ptr), _p(fill[f]), fill[f].nbytes))

    def refused(code, **ch):
        a = dict(zip(names, good)); a.update(ch)
        assert raw(*[a[n] for n in names]) == code, ch
        assert lib().lvk_last_error(ctx.h)                                       # a message, not an empty string
        untouched(ch)                                                            # nothing was launched
        assert raw(*good) == LVK_OK                                              # the context goes on
        is_the_reference(ch)

    for ch in (dict(d_md=None), dict(d_cd=None), dict(d_best=None), dict(d_sel=None), dict(d_info=None), dict(n_map=-1), dict(n_cand=-1),
               dict(max_dist=-1), dict(max_dist=257), dict(ratio_pct=0), dict(ratio_pct=101), dict(max_matches=0), dict(max_matches=1025),
               dict(d_md=d_md.ptr + 4), dict(d_cd=d_cd.ptr + 1)):
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n_cand=4097)
    refused(LVK_ERR_CAPACITY, n_map=(1 << 20) + 1)
    # n_cand == 0: fine, nothing is launched and nothing is written; null pointers are allowed where the count is zero
    assert raw(d_md, nm, None, 0, 58, 100, 1024, None, None, None) == LVK_OK
    untouched("n_cand == 0")
    # n_map == 0: every corner NO_CANDIDATE, the counts say so, nothing is selected
    assert raw(None, 0, d_cd, nc, 58, 100, 1024, d["best"], d["sel"], d["info"]) == LVK_OK
    got = read()
    best = got["best"].view(MATCH_RESULT); info = got["info"].view(GLOBAL_INFO)[0]
    assert (best["status"] == R.NO_CANDIDATE).all() and (best["cand"] == -1).all() and (best["n_window"] == 0).all() and (best["pad"] == 0).all()
    assert info["n_no_candidate"] == nc and info["n_selected"] == 0 and info["n_ok"] == 0 and (got["sel"] == 0x5A).all()
