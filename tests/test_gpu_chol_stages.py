"""Stage tests of the default update route's factor-and-solve (k_chol_fused and the 160-row recursion of launch_chol_solve,
larvio_amd/csrc/be_linalg.hip) through lvk_chol_solve, against the long-double restatement of tests/chol_ref.py: W = L^-1 B, the Gram
matrix G = W^T W the update consumes, and the blocks of L the kernel stores, each entry within the bound derived there.  The problems,
their seeds and the side condition are chol_ref's (tests/test_chol_ref.py checks them on the CPU); references are cached there."""
import numpy as np
import pytest

from tests import chol_ref as R

pytestmark = pytest.mark.gpu

FILTER_LDS = 1032                                            # the filter's workspace stride: rows_cap + 8


def _packed(S, B):
    """S in rows of (m + 7) & ~7 doubles, B in rows of exactly nbcols; NaN padding"""
    from larvio_amd import larvio as lv
    m = S.shape[0]
    return lv._padded(S, (m + 7) & ~7), np.array(B)


def _run(ctx, Sbuf, m, Bbuf, nbcols):
    from larvio_amd import larvio as lv
    return lv.chol_solve(ctx, Sbuf, m, Bbuf, nbcols)


def _check(Sout, Bout, m, nbcols, ref, bnd, what):
    rW, rG, rL = R.ratios(Bout[:m, :nbcols], R.extract_L(Sout, m), ref, bnd)
    print(f"{what}: worst |error| / bound: W {rW:.3e}  G {rG:.3e}  L {rL:.3e}")
    assert rW <= 1.0 and rG <= 1.0 and rL <= 1.0, (what, rW, rG, rL)
    return rW, rG, rL


@pytest.mark.parametrize("m,nbcols", R.ALL_CASES)
def test_chol_solve_within_the_derived_bound(gpu_ctx, m, nbcols):
    """panel count (m = 1 .. 160 at nbcols = 33), solver grid and wavefront exit (nbcols = 1 .. 129 at m = 65), recursion and second
    right-hand side (rest = m - 160 = 1 .. 65, 160, 161; m = 481: three super-blocks)"""
    S, B, ref, bnd = R.find_problem(m, nbcols)
    Sb, Bb = _packed(S, B)
    Sout, Bout, info = _run(gpu_ctx, Sb, m, Bb, nbcols)
    assert info == (0, 0)
    assert np.array_equal(Sout[:, m:].view(np.uint64), Sb[:, m:].view(np.uint64))
    _check(Sout, Bout, m, nbcols, ref, bnd, f"m {m} nbcols {nbcols}")


def _unread_mask(m):
    """True where lvk_chol_solve's header comment says S is not read (m x m part): below-left of a super-block; inside a super-block
    above the diagonal 32 x 32 blocks; of a diagonal block the tile above-right of its diagonal tiles and the strict LOWER triangle of
    the two 16 x 16 diagonal tiles"""
    r = np.arange(m)[:, None]; c = np.arange(m)[None, :]
    sb_r, sb_c = r // R.MB, c // R.MB
    same_sb = sb_r == sb_c
    same_blk = (r // 32) == (c // 32)
    same_tile = (r // 16) == (c // 16)
    return (sb_r > sb_c) | (same_sb & ~same_blk & (c > r)) | (same_blk & ~same_tile & (c > r)) | (same_tile & (r > c))


@pytest.mark.parametrize("m,nbcols", R.STRIDED_CASES)
def test_chol_solve_at_the_filters_strides(gpu_ctx, m, nbcols):
    """lds = 1032 and ldb an odd multiple of 8, NaN in the padding AND in every entry of S the header says is not read: bit-identical
    to the packed call on everything defined, padding untouched"""
    S, B, ref, bnd = R.find_problem(m, nbcols)
    Sb, Bb = _packed(S, B)
    S0, B0, info0 = _run(gpu_ctx, Sb, m, Bb, nbcols)
    ldb = ((nbcols + 7) & ~7) | 8
    Ss = np.full((m, FILTER_LDS), np.nan); Ss[:, :m] = np.where(_unread_mask(m), np.nan, S)
    Bs = np.full((m, ldb), np.nan); Bs[:, :nbcols] = B
    S1, B1, info1 = _run(gpu_ctx, Ss, m, Bs, nbcols)
    assert info0 == (0, 0) and info1 == (0, 0)
    assert np.array_equal(B1[:, :nbcols].view(np.uint64), B0[:, :nbcols].view(np.uint64))
    assert np.array_equal(R.extract_L(S1, m).view(np.uint64), R.extract_L(S0, m).view(np.uint64))
    nanbits = np.array(np.nan).view(np.uint64)
    assert (S1[:, m:].view(np.uint64) == nanbits).all() and (B1[:, nbcols:].view(np.uint64) == nanbits).all()
    _check(S1, B1, m, nbcols, ref, bnd, f"strided m {m} nbcols {nbcols}")


@pytest.mark.parametrize("bad", R.REPORT_BAD)
def test_chol_solve_reports_the_first_non_positive_pivot(gpu_ctx, bad):
    S, B = R.indefinite_problem(bad)
    Sb, Bb = _packed(S, B)
    _, _, info = _run(gpu_ctx, Sb, R.REPORT_M, Bb, R.REPORT_NB)
    assert info == (bad + 1, 0), info
    # the context (flags, epoch, report words) is as good as new
    m, nbcols = 193, 33
    S, B, ref, bnd = R.find_problem(m, nbcols)
    Sb, Bb = _packed(S, B)
    Sout, Bout, info = _run(gpu_ctx, Sb, m, Bb, nbcols)
    assert info == (0, 0)
    _check(Sout, Bout, m, nbcols, ref, bnd, f"after bad pivot {bad}: m {m} nbcols {nbcols}")


def test_chol_solve_repeats_bit_identically_across_sizes(gpu_ctx):
    """the flag / epoch protocol: every shape in one context, large to small, small to large, large to small again; each repeat
    equals its first run bit for bit (a stale flag or a stale Y block from another size would show)"""
    order = sorted(R.ALL_CASES, key=lambda c: (-c[0], -c[1]))
    first = {}
    for case in order + order[::-1] + order:
        m, nbcols = case
        S, B, _, _ = R.find_problem(m, nbcols)
        Sb, Bb = _packed(S, B)
        Sout, Bout, info = _run(gpu_ctx, Sb, m, Bb, nbcols)
        assert info == (0, 0)
        got = (R.extract_L(Sout, m).view(np.uint64), Bout.view(np.uint64))
        if case not in first:
            first[case] = got
        else:
            assert np.array_equal(got[0], first[case][0]) and np.array_equal(got[1], first[case][1]), case


def test_chol_solve_checks_its_arguments(gpu_ctx):
    from larvio_amd import larvio as lv
    from larvio_amd._lib import lib
    lv._L()
    m, nbcols = 33, 17
    S, B, ref, bnd = R.find_problem(33, 33)
    B = B[:, :nbcols]
    Sb = lv._padded(S, 40); Bb = np.array(B)
    dS, dB = gpu_ctx.to_device(Sb), gpu_ctx.to_device(Bb)
    info = np.zeros(2, np.int32)
    f = lib().lvk_chol_solve
    args = lambda **k: [k.get(a, d) for a, d in (("ctx", gpu_ctx.h), ("S", lv._p(dS)), ("lds", 40), ("m", m), ("B", lv._p(dB)), ("ldb", nbcols), ("nb", nbcols), ("info", lv._p(info)))]
    assert f(*args(lds=32)) == 1                              # lds < m
    assert f(*args(lds=38)) == 1                              # not a multiple of 4
    assert f(*args(ldb=16)) == 1                              # ldb < nbcols
    assert f(*args(m=-1)) == 1 and f(*args(nb=-1)) == 1
    assert f(*args(S=lv._p(dS.ptr + 8))) == 1                 # rows would not start 32-byte aligned
    assert f(*args(S=None)) == 1 and f(*args(B=None)) == 1 and f(*args(info=None)) == 1
    # nothing was launched: the buffers are as they were, and the same context then solves the problem
    assert np.array_equal(gpu_ctx.to_host(dS, np.float64, Sb.shape).view(np.uint64), Sb.view(np.uint64))
    assert np.array_equal(gpu_ctx.to_host(dB, np.float64, Bb.shape), Bb)
    info[:] = 9
    assert f(*args(m=0)) == 0 and info.tolist() == [0, 0]
    gpu_ctx.check(f(*args()))
    assert info.tolist() == [0, 0]
    Wc = gpu_ctx.to_host(dB, np.float64, Bb.shape)
    assert (np.abs(np.asarray(Wc, R.LD) - ref["W"][:, :nbcols]) <= bnd["W"][:, :nbcols]).all()
