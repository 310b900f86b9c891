"""Stage tests of the FP64 matrix-core GEMM (k_dgemm_sk, larvio_amd/csrc/be_linalg.hip) through lvk_dgemm and lvk_dgemm_ex: all four
transpose instantiations at the K edges of its split (kc changes at 64 / 65, 128 / 129, 192 / 193; K = 0 .. 3 leave whole wavefronts
without work), against a long-double product with a componentwise bound, on operands whose rows and columns are scaled over
1e-8 .. 1 so that a wrong entry in a small block cannot hide behind a large one; the riders the update uses; argument refusals.

The bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (3.5): a K-term dot product in ANY order, so the split
into four partial sums and their fixed-order addition are covered):
    |fl(alpha op(A) op(B) + beta C) - exact| <= gamma_K |alpha| |A||B|  +  u |alpha| |A||B|  (the product with alpha, unless alpha = +-1)
                                              +  u |beta C|  (the product with beta, unless beta = 0 or +-1)
                                              +  u |result|  (the last addition; once more when diag_add is added)
which is gamma_K |A||B| + u |result| for alpha = 1, beta = 0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SHAPES = [(17, 5, 33), (16, 16, 64), (15, 17, 65), (33, 47, 128), (33, 47, 129), (20, 20, 256), (20, 20, 257), (5, 3, 1), (5, 3, 3), (7, 9, 0)]
TRANS = [(False, False), (False, True), (True, False), (True, True)]


def _gamma(k):
    return k * U / (1.0 - k * U)


def _scaled(rng, r, c):
    return rng.normal(0, 1, (r, c)) * (10.0 ** rng.uniform(-8, 0, r))[:, None] * (10.0 ** rng.uniform(-8, 0, c))[None, :]


def _operands(seed, M, N, K, ta, tb):
    rng = np.random.default_rng(seed)
    return _scaled(rng, *((K, M) if ta else (M, K))), _scaled(rng, *((N, K) if tb else (K, N))), _scaled(rng, M, N)


def _ref_and_bound(A, B, C0, ta, tb, alpha, beta, diag_add=0.0):
    oA = np.asarray(A.T if ta else A, LD); oB = np.asarray(B.T if tb else B, LD)
    K = oA.shape[1]
    prod = oA @ oB
    ref = LD(alpha) * prod + (LD(beta) * np.asarray(C0, LD) if beta != 0 else 0)
    if diag_add:
        ref = ref + LD(diag_add) * np.eye(*ref.shape, dtype=LD)
    ab = np.abs(oA) @ np.abs(oB)
    bound = _gamma(K) * abs(alpha) * ab + U * np.abs(ref)
    if abs(alpha) not in (0.0, 1.0):
        bound = bound + U * abs(alpha) * ab
    if abs(beta) not in (0.0, 1.0):
        bound = bound + U * np.abs(LD(beta) * np.asarray(C0, LD))
    if diag_add:
        bound = bound + U * np.abs(ref)
    return ref, bound, prod, _gamma(K) * ab


def _worst(out, ref, bound, what):
    e = np.abs(np.asarray(out, LD) - ref)
    ratio = float(np.max(np.where(bound > 0, e / np.where(bound > 0, bound, 1), np.where(e > 0, np.inf, 0)))) if e.size else 0.0
    print(f"{what}: worst |error| / bound {ratio:.3e}")
    assert ratio <= 1.0, (what, ratio)
    return ratio


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dgemm_within_the_componentwise_bound(gpu_ctx, shape, ta, tb):
    from larvio_amd import larvio as lv
    M, N, K = shape
    A, B, C0 = _operands(1000 * M + 10 * K + 2 * ta + tb, M, N, K, ta, tb)
    ref, bound, _, _ = _ref_and_bound(A, B, C0, ta, tb, 0.7, -0.3)
    out = lv.dgemm(gpu_ctx, A, B, ta, tb, alpha=0.7, beta=-0.3, Cin=C0)
    _worst(out, ref, bound, f"dgemm {shape} ta {int(ta)} tb {int(tb)}")
    # beta = 0 never reads C: NaN there does not reach the result (K = 0: C = 0)
    ref0, bound0, _, _ = _ref_and_bound(A, B, C0, ta, tb, 1.0, 0.0)
    out0 = lv.dgemm(gpu_ctx, A, B, ta, tb, alpha=1.0, beta=0.0, Cin=np.full((M, N), np.nan))
    assert np.isfinite(out0).all()
    _worst(out0, ref0, bound0, f"dgemm beta 0 over NaN {shape} ta {int(ta)} tb {int(tb)}")
    # alpha = 0: C = beta C, one rounding
    outa = lv.dgemm(gpu_ctx, A, B, ta, tb, alpha=0.0, beta=-0.3, Cin=C0)
    assert np.array_equal(outa, -0.3 * C0)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_identity_returns_an_asymmetric_B_exactly(gpu_ctx, ta, tb):
    """a row/column swap in the accumulator map or a transposed operand read shows as a wrong entry, not as rounding"""
    from larvio_amd import larvio as lv
    M, N = 20, 13
    _, B, _ = _operands(7 + 2 * ta + tb, M, N, M, ta, tb)
    out = lv.dgemm(gpu_ctx, np.eye(M), B, ta, tb)
    assert np.array_equal(out, B.T if tb else B)


@pytest.mark.parametrize("M,N", [(21, 21), (21, 19), (19, 37)])
def test_dgemm_ex_diag_add_lands_on_the_diagonal_only(gpu_ctx, M, N):
    from larvio_amd import larvio as lv
    K = 7
    A, B, C0 = _operands(M + N, M, N, K, False, True)
    ref, bound, _, _ = _ref_and_bound(A, B, C0, False, True, 1.0, 0.0, diag_add=0.25)
    out, _ = lv.dgemm_ex(gpu_ctx, A, B, np.full((M, N), np.nan), M, N, K, transb=True, diag_add=0.25)
    _worst(out, ref, bound, f"diag_add {M} x {N}")
    plain = lv.dgemm(gpu_ctx, A, B, False, True)
    off = ~np.eye(M, N, dtype=bool)
    assert np.array_equal(out[off], plain[off]) and np.array_equal(out[~off], plain[~off] + 0.25)


def test_dgemm_ex_xin_fills_its_column_for_every_row(gpu_ctx):
    """[H P | r] in one launch: M = 21 rows (the last tile is partial), the column right of the N computed ones"""
    from larvio_amd import larvio as lv
    M, N, K, ldc = 21, 19, 10, 24
    A, B, _ = _operands(3, M, N, K, False, False)
    xin = np.random.default_rng(4).normal(0, 1, M)
    out, _ = lv.dgemm_ex(gpu_ctx, A, B, np.full((M, ldc), np.nan), M, N, K, xin=xin, xin_col=N)
    assert np.array_equal(out[:, N], xin)
    assert np.array_equal(out[:, :N], lv.dgemm(gpu_ctx, A, B))
    assert np.isnan(out[:, N + 1:]).all()


@pytest.mark.parametrize("xout_col", [17, 18, 0])
def test_dgemm_ex_xout_diverts_one_column_unscaled(gpu_ctx, xout_col):
    """W^T [W | w] of the update: alpha = -1, beta = 1; the diverted column is the plain sum, its place in C keeps its old bits.
    Columns 17 and 18 lie in the partial tile of N = 19."""
    from larvio_amd import larvio as lv
    M, N, K = 21, 19, 33
    A, B, C0 = _operands(5 + xout_col, M, N, K, True, False)
    ref, bound, prod, bprod = _ref_and_bound(A, B, C0, True, False, -1.0, 1.0)
    out, xout = lv.dgemm_ex(gpu_ctx, A, B, C0, M, N, K, transa=True, alpha=-1.0, beta=1.0, xout=np.full(M, np.nan), xout_col=xout_col)
    keep = np.arange(N) != xout_col
    _worst(out[:, keep], ref[:, keep], bound[:, keep], f"xout {xout_col}: C")
    _worst(xout, prod[:, xout_col], bprod[:, xout_col], f"xout {xout_col}: diverted column")
    assert np.array_equal(out[:, xout_col].view(np.uint64), C0[:, xout_col].view(np.uint64))


@pytest.mark.parametrize("gate", [(3, 0), (0, 161)])
def test_dgemm_ex_set_gate_leaves_everything_as_it_was(gpu_ctx, gate):
    from larvio_amd import larvio as lv
    M, N, K = 21, 19, 33
    A, B, C0 = _operands(11, M, N, K, True, False)
    C0[2, 3] = np.nan
    x0 = np.full(M, 7.25)
    out, xout = lv.dgemm_ex(gpu_ctx, A, B, C0, M, N, K, transa=True, alpha=-1.0, beta=1.0, xout=x0, xout_col=18, gate=gate)
    assert np.array_equal(out.view(np.uint64), C0.view(np.uint64)) and np.array_equal(xout, x0)
    # an open gate changes nothing about the product
    C0[2, 3] = 0.5
    a, xa = lv.dgemm_ex(gpu_ctx, A, B, C0, M, N, K, transa=True, alpha=-1.0, beta=1.0, xout=x0, xout_col=18, gate=(0, 0))
    b, xb = lv.dgemm_ex(gpu_ctx, A, B, C0, M, N, K, transa=True, alpha=-1.0, beta=1.0, xout=x0, xout_col=18)
    assert np.array_equal(a, b) and np.array_equal(xa, xb) and not np.array_equal(a, C0)


def test_dgemm_entries_check_their_arguments(gpu_ctx):
    import ctypes as C
    from larvio_amd import larvio as lv
    from larvio_amd._lib import lib
    lv._L()
    M, N, K = 5, 7, 9
    A, B, C0 = _operands(1, M, N, K, False, False)
    dA, dB, dC, dx = gpu_ctx.to_device(np.zeros((16, 16))), gpu_ctx.to_device(np.zeros((16, 16))), gpu_ctx.to_device(np.full((16, 16), 2.5)), gpu_ctx.to_device(np.zeros(16))
    one, zero = C.c_double(1.0), C.c_double(0.0)

    def plain(ta, tb, M, N, K, lda, ldb, ldc, A=dA, B=dB, Cm=dC):
        return lib().lvk_dgemm(gpu_ctx.h, ta, tb, M, N, K, one, lv._p(A), lda, lv._p(B), ldb, zero, lv._p(Cm), ldc)

    def ex(ta, tb, M, N, K, lda, ldb, ldc, xin=None, xin_col=0, xout=None, xout_col=0):
        return lib().lvk_dgemm_ex(gpu_ctx.h, ta, tb, M, N, K, one, lv._p(dA), lda, lv._p(dB), ldb, zero, lv._p(dC), ldc, zero, lv._p(xin), xin_col, lv._p(xout), xout_col, None)
    for f in (plain, ex):
        assert f(0, 0, -1, N, K, 16, 16, 16) == 1 and f(0, 0, M, -1, K, 16, 16, 16) == 1 and f(0, 0, M, N, -1, 16, 16, 16) == 1
        assert f(0, 0, M, N, K, K - 1, 16, 16) == 1 and f(0, 0, M, N, K, K, N, N) == 0          # A stored M x K
        assert f(1, 0, M, N, K, M - 1, 16, 16) == 1 and f(1, 0, M, N, K, M, N, N) == 0          # A stored K x M
        assert f(0, 0, M, N, K, 16, N - 1, 16) == 1                                             # B stored K x N
        assert f(0, 1, M, N, K, 16, K - 1, 16) == 1 and f(0, 1, M, N, K, K, K, N) == 0          # B stored N x K
        assert f(0, 0, M, N, K, 16, 16, N - 1) == 1
    assert plain(0, 0, M, N, K, 16, 16, 16, A=None) == 1 and plain(0, 0, M, N, K, 16, 16, 16, Cm=None) == 1
    assert ex(0, 0, M, N, K, 16, 16, 16, xin=dx, xin_col=16) == 1 and ex(0, 0, M, N, K, 16, 16, 16, xin=dx, xin_col=-1) == 1
    assert ex(0, 0, M, N, K, 16, 16, 16, xout=dx, xout_col=N) == 1 and ex(0, 0, M, N, K, 16, 16, 16, xout=dx, xout_col=-1) == 1
    # K = 0 is legal: C = beta C (here beta = 0); and the context still works after the refusals
    assert plain(0, 0, M, N, 0, 0, 16, 16) == 0
    got = gpu_ctx.to_host(dC, np.float64, (16, 16))
    assert np.array_equal(got[:M, :N], np.zeros((M, N))) and np.array_equal(got[M:], np.full((16 - M, 16), 2.5))
    ref, bound, _, _ = _ref_and_bound(A, B, C0, False, False, 1.0, 0.0)
    _worst(lv.dgemm(gpu_ctx, A, B), ref, bound, "after the refusals")
