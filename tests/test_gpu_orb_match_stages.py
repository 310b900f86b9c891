"""GPU: the guided ORB matcher's stage entry (lvk_orb_match_guided) on every case of tests/orb_match_cases.py - each result must be the
restatement's (tests/orb_match_ref.py, held to a brute-force loop by tests/test_orb_match_ref.py), field for field, pad included - and its
refusals, each followed by a good call on the same context."""
import ctypes as C

import numpy as np
import pytest

from larvio_amd import ops
from larvio_amd._lib import lib, _p, MATCH_QUERY, MATCH_RESULT
from tests import orb_match_cases as MC
from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3


def _run(ctx, k, **over):
    a = dict(max_dist=k["max_dist"], ratio_pct=k["ratio_pct"]); a.update(over)
    return ops.orb_match_guided(ctx, k["cand_pts"], k["cand_desc"], k["q_px"], k["q_radius"], k["q_desc"], **a)


@pytest.mark.parametrize("name", list(MC.cases()))
def test_case_equals_the_restatement(gpu_ctx, name):
    got = _run(gpu_ctx, MC.cases()[name])
    want = MC.reference(name)
    for f in R.RESULT.names:
        assert np.array_equal(got[f], want[f]), (name, f, np.nonzero(got[f] != want[f])[0][:8])
    assert got.tobytes() == want.tobytes()
    MC.check_want(name, got)


def test_a_second_call_starts_from_clean_claims(gpu_ctx):
    """the claim words live in the context's scratch: a pile-up must not leak into the next call"""
    _run(gpu_ctx, MC.cases()["pile_up_1024"])
    for name in ("conflict_two_equal", "random_c65_q64"):
        assert _run(gpu_ctx, MC.cases()[name]).tobytes() == MC.reference(name).tobytes()


def _raw(ctx, d_cp, d_cd, n_cand, d_q, d_qd, n_q, max_dist, ratio_pct, d_out):
    return lib().lvk_orb_match_guided(ctx.h, _p(d_cp), _p(d_cd), n_cand, _p(d_q), _p(d_qd), n_q, max_dist, ratio_pct, _p(d_out))


def test_refusals_leave_the_context_usable(gpu_ctx):
    ctx = gpu_ctx
    k = MC.cases()["random_c65_q64"]
    q = np.zeros(64, MATCH_QUERY); q["x"] = k["q_px"][:, 0]; q["y"] = k["q_px"][:, 1]; q["radius"] = k["q_radius"]
    fill = np.zeros(64, MATCH_RESULT); fill.view(np.uint8)[...] = 0x5A
    d_cp = ctx.to_device(k["cand_pts"]); d_q = ctx.to_device(q); d_out = ctx.to_device(fill)
    d_cd = ctx.to_device(np.concatenate([k["cand_desc"].ravel(), np.zeros(8, np.uint8)]))
    d_qd = ctx.to_device(np.concatenate([k["q_desc"].ravel(), np.zeros(8, np.uint8)]))
    good = (d_cp, d_cd, 65, d_q, d_qd, 64, 58, 100, d_out)

    def refused(code, **ch):
        names = ("d_cp", "d_cd", "n_cand", "d_q", "d_qd", "n_q", "max_dist", "ratio_pct", "d_out")
        a = dict(zip(names, good)); a.update(ch)
        assert _raw(ctx, *[a[n] for n in names]) == code, ch
        assert lib().lvk_last_error(ctx.h)                                       # a message, not an empty string
        ctx.sync()
        assert ctx.to_host(d_out, MATCH_RESULT, (64,)).tobytes() == fill.tobytes(), ch   # nothing was launched
        assert _raw(ctx, *good) == LVK_OK                                        # the context goes on
        assert ctx.to_host(d_out, MATCH_RESULT, (64,)).tobytes() == MC.reference("random_c65_q64").tobytes(), ch
        ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(d_out.ptr), _p(fill), fill.nbytes))

    for ch in (dict(d_cp=None), dict(d_cd=None), dict(d_q=None), dict(d_qd=None), dict(d_out=None), dict(n_cand=-1), dict(n_q=-1),
               dict(max_dist=-1), dict(max_dist=257), dict(ratio_pct=0), dict(ratio_pct=101), dict(d_cd=d_cd.ptr + 4), dict(d_qd=d_qd.ptr + 1)):
        refused(LVK_ERR_ARG, **ch)
    refused(LVK_ERR_CAPACITY, n_cand=4097)
    refused(LVK_ERR_CAPACITY, n_q=1025)
    # n_q == 0: fine, and nothing is written; null pointers are allowed where the count is zero
    assert _raw(ctx, d_cp, d_cd, 65, None, None, 0, 58, 100, None) == LVK_OK
    ctx.sync()
    assert ctx.to_host(d_out, MATCH_RESULT, (64,)).tobytes() == fill.tobytes()
    assert _raw(ctx, None, None, 0, d_q, d_qd, 64, 58, 100, d_out) == LVK_OK
    got = ctx.to_host(d_out, MATCH_RESULT, (64,))
    assert (got["status"] == R.NO_CANDIDATE).all() and (got["cand"] == -1).all() and (got["n_window"] == 0).all() and (got["pad"] == 0).all()
