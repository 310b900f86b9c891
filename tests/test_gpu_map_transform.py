"""GPU: lvk_map_transform (ops.map_transform) against larvio_amd.localize.transform_points, the numpy statement of the header's expressions in
the header's order - bit for bit, at n = 1, 255, 256, 257, 1000 (one lane, one under / exactly / one over a chunk of 256, several chunks), with
and without covariances, descriptors, the alignment's covariance and the alignment itself, the outputs written as the tails of larger
buffers whose heads and guard bytes must stay, a NaN and an infinite point passing through, and every refusal launching nothing."""
import ctypes as C
import itertools

import numpy as np
import pytest

from larvio_amd import localize as L
from larvio_amd import ops
from larvio_amd._lib import lib, _p

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG, LVK_ERR_CAPACITY = 0, 1, 3
SIZES = (1, 255, 256, 257, 1000)


def _data(n, seed=0):
    rng = np.random.default_rng([20261203, seed, n])
    X = rng.uniform(-50.0, 50.0, (n, 3))
    M = rng.normal(size=(n, 3, 3)); cov = 1e-4 * (M @ M.transpose(0, 2, 1))
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    psi = 0.7
    al = dict(c=np.cos(psi), s=np.sin(psi), t=np.array([3.0, -2.0, 0.4]))
    Q = rng.normal(size=(4, 4)); P = 1e-5 * (Q @ Q.T)
    return X, cov, desc, al, P


def _same(got, want):
    """bit for bit where the judge is finite; where it is not, the same kind of non-finite (a NaN's payload is the hardware's own)"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return got.shape == want.shape and got[fin].tobytes() == want[fin].tobytes() and np.array_equal(got[~fin], want[~fin], equal_nan=True)


@pytest.mark.parametrize("n", SIZES)
def test_every_combination_is_numpy_bit_for_bit_and_the_heads_and_guards_stay(gpu_ctx, n):
    X, cov, desc, al, P = _data(n)
    G = ops.MAP_TRANSFORM_GUARD
    for use_cov, use_desc, use_P, use_al in itertools.product((False, True), repeat=4):
        head = 3 if use_desc else 0
        out = ops.map_transform(gpu_ctx, X, cov if use_cov else None, desc if use_desc else None, (al["c"], al["s"], al["t"]) if use_al else None, P if use_P else None, head=head)
        p, w = L.transform_points(X, cov if use_cov else None, al if use_al else None, P if use_P else None)
        what = (n, use_cov, use_desc, use_P, use_al)
        assert out["X"].tobytes() == p.tobytes(), what
        assert out["X"].tobytes() == L.apply_alignment(al if use_al else dict(c=1.0, s=0.0, t=np.zeros(3)), X)[0].tobytes(), what
        if w is None:
            assert out["cov"] is None and (out["cov_raw"] == 0xA5).all(), what                    # nothing asked for: nothing written
        else:
            assert out["cov"].tobytes() == w.tobytes(), what
            assert out["cov"].tobytes() == out["cov"].transpose(0, 2, 1).copy().tobytes()          # the lower triangle is a copy
        if use_desc:
            assert out["desc"].tobytes() == desc.tobytes(), what
        else:
            assert out["desc"] is None and (out["desc_raw"] == 0xA5).all(), what
        for k, rec in (("X", 24), ("cov", 72), ("desc", 32)):
            raw = out[k + "_raw"]
            assert (raw[:rec * head] == 0xA5).all() and (raw[-G:] == 0xA5).all(), (what, k)        # the head of the larger buffer, and what lies behind the tail


def test_null_alignment_is_the_identity_record_and_non_finite_inputs_pass_through(gpu_ctx):
    X, cov, desc, al, P = _data(300, 1)
    a = ops.map_transform(gpu_ctx, X, cov, desc, None, P); b = ops.map_transform(gpu_ctx, X, cov, desc, (1.0, 0.0, np.zeros(3)), P)
    assert a["X"].tobytes() == b["X"].tobytes() and a["cov"].tobytes() == b["cov"].tobytes()
    X[5, 0] = np.nan; X[17, 1] = np.inf; X[256, 2] = -np.inf; cov[9, 1, 1] = np.nan; cov[40, 0, 2] = np.inf
    out = ops.map_transform(gpu_ctx, X, cov, desc, (al["c"], al["s"], al["t"]), P)
    p, w = L.transform_points(X, cov, al, P)
    assert _same(out["X"], p) and _same(out["cov"], w) and out["desc"].tobytes() == desc.tobytes()
    assert np.isnan(out["X"][5, :2]).all() and out["X"][5, 2] == p[5, 2] and not np.isfinite(out["X"][17, :2]).any() and out["X"][256, 2] == -np.inf
    assert not np.isfinite(out["cov"][9]).all() and not np.isfinite(out["cov"][40]).all()
    rest = np.ones(300, bool); rest[[5, 17, 256, 9, 40]] = False
    assert np.isfinite(out["X"][rest]).all() and np.isfinite(out["cov"][rest]).all()              # and nobody else is touched by them


def test_refusals_launch_nothing_and_the_context_goes_on(gpu_ctx):
    ctx = gpu_ctx
    X, cov, desc, al, P = _data(64, 2)
    rec = ops.align_record((al["c"], al["s"], al["t"]))
    d_X = ctx.to_device(X); d_cov = ctx.to_device(cov.reshape(-1, 9)); d_desc = ctx.to_device(desc)
    fills = dict(X=np.full(24 * 64, 0x5A, np.uint8), cov=np.full(72 * 64, 0x5A, np.uint8), desc=np.full(32 * 64, 0x5A, np.uint8))
    outs = {k: ctx.to_device(v) for k, v in fills.items()}
    good = dict(X=d_X, cov=d_cov, desc=d_desc, n=64, al=rec, P=np.ascontiguousarray(P).reshape(16), oX=outs["X"], ocov=outs["cov"], odesc=outs["desc"])

    def raw(a):
        return lib().lvk_map_transform(ctx.h, _p(a["X"]), _p(a["cov"]), _p(a["desc"]), a["n"], _p(a["al"]), _p(a["P"]), _p(a["oX"]), _p(a["ocov"]), _p(a["odesc"]))

    def read():
        ctx.sync()
        return tuple(ctx.to_host(outs[k], np.uint8, fills[k].shape).tobytes() for k in ("X", "cov", "desc"))
    untouched = tuple(fills[k].tobytes() for k in ("X", "cov", "desc"))
    p, w = L.transform_points(X, cov, al, P)
    done = (p.tobytes(), w.tobytes(), desc.tobytes())
    bad_al = rec.copy(); bad_al["t"][0, 1] = np.nan
    bad_c = rec.copy(); bad_c["c"] = np.inf
    bad_P = good["P"].copy(); bad_P[7] = np.nan
    for code, ch in ((LVK_ERR_ARG, dict(X=None)), (LVK_ERR_ARG, dict(oX=None)), (LVK_ERR_ARG, dict(ocov=None)), (LVK_ERR_ARG, dict(odesc=None)), (LVK_ERR_ARG, dict(n=-1)),
                     (LVK_ERR_ARG, dict(al=bad_al)), (LVK_ERR_ARG, dict(al=bad_c)), (LVK_ERR_ARG, dict(P=bad_P)), (LVK_ERR_ARG, dict(cov=None, P=None, ocov=None, odesc=outs["desc"].ptr + 4)),
                     (LVK_ERR_ARG, dict(desc=d_desc.ptr + 4)), (LVK_ERR_CAPACITY, dict(n=(1 << 20) + 1))):
        a = dict(good); a.update(ch)
        assert raw(a) == code, ch
        assert lib().lvk_last_error(ctx.h)
        assert read() == untouched, ch                                                              # nothing was launched
        assert raw(good) == LVK_OK and read() == done, ch                                           # the context goes on
        for k in fills:
            ctx.check(lib().lvk_memcpy_h2d(ctx.h, C.c_void_p(outs[k].ptr), _p(fills[k]), fills[k].nbytes))
    a = dict(good); a.update(n=0, X=None, oX=None, ocov=None, odesc=None, cov=None, desc=None)
    assert raw(a) == LVK_OK and read() == untouched                                                 # n == 0: LVK_OK, nothing launched
    a = dict(good); a.update(cov=None, P=None, ocov=None)
    assert raw(a) == LVK_OK and read() == (done[0], untouched[1], done[2])                          # no covariance asked for: none needed, none written
