"""Stage tests of the measurement-row compressions: lvk_ekf_compress_qr_groups (be_qr.hip: the register node kernel k_qr_sparse_reg in
both specialisations and the LDS node kernel k_qr_sparse) and lvk_ekf_compress_qr (be_qr_dense.hip: CAQR), each against LAPACK
Householder QR of the same compression, pair by pair in the column-scaled measure of tests/qr_ref.py:

    max_ij |G_kernel - G|_ij / (c_i c_j) <= 10 max(tau_ref, cols u)

with tau_ref the reference's own worst pair on the case (tests/test_qr_ref.py checks on the CPU that it stays <= 1e-12 and that every
case lands on the kernel and specialisation it names).  H's columns are scaled by 10^U(-4, 4) so that the small columns count.
Each test prints tau_ref, the kernel's worst pair and their ratio.  Also: the structural claims of the node outputs, an exactly zero
strict lower triangle of the dense result, the filter's padded leading dimension (bit-identical results, padding untouched), the
dense capacity, and the negligible-column rule (QR_NEGLIGIBLE) in each of the three reflector kernels."""
import ctypes as C

import numpy as np
import pytest

from tests import qr_ref as Q

pytestmark = pytest.mark.gpu


def _filter_ld(n):
    return ((n + 15) & ~15) + 8                  # the filter's padded leading dimension (backend.hip, lvk_ekf_create)


def _errors(name, H, r, Hc, rc, Href, rref):
    """-> (e of the kernel, bound); prints tau_ref, the kernel's worst pair and their ratio"""
    G, c = Q.gram(H, r), Q.col_norms(H, r)
    tau = Q.pair_errors(Q.gram(Href, rref), G, c).max()
    e = Q.pair_errors(Q.gram(Hc, rc), G, c)
    b = Q.bound(tau, H.shape[1])
    print(f"QRSTAGE {name}: tau_ref {tau:.3e} kernel {e.max():.3e} ratio {e.max() / tau if tau > 0 else float('inf'):.2f} bound {b:.3e}")
    return e, b


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# --------------------------------------------------------------------------------------------------- structure-aware path
@pytest.mark.parametrize("name", Q.GROUP_CASES)
def test_compress_qr_groups_stage(gpu_ctx, name):
    """one register node per case at the kernel's edges (RPL 8 / 16, chunk handovers, column quads), mixed levels with copy blocks,
    a three-level plan, and the LDS kernel (wider than 63 columns, taller than 256 rows, with and without the LDS opt-in, and the
    gate-rejection pattern as one 300-row group)"""
    from larvio_amd import larvio as lv
    c = Q.group_case(name)
    H, r = c["H"], c["r"]
    levels, final_rows = lv.qr_plan(c["N"], c["groups"])
    Hc, rc = lv.compress_qr_groups(gpu_ctx, H, r, c["groups"])
    assert len(Hc) == final_rows < len(H)
    assert np.isfinite(Hc).all() and np.isfinite(rc).all()
    bad = Q.structural_violations(levels, H, r, Hc, rc)
    assert not bad, bad[:8]
    Href, rref = Q.emulate(levels, H, r)
    e, b = _errors(name, H, r, Hc, rc, Href, rref)
    assert e.max() <= b, np.unravel_index(np.argmax(e), e.shape)


# --------------------------------------------------------------------------------------------------- dense path
@pytest.mark.parametrize("rows,cols", Q.DENSE)
def test_compress_qr_dense_stage(gpu_ctx, rows, cols):
    """CAQR at its chunk edges (CH = 512 / 1024), a chunk count that changes between panels, panel edges, few rows in the last panel
    and the 65,536-row capacity: within the bound, and k_caqr_clean leaves an exactly zero strict lower triangle"""
    from larvio_amd import larvio as lv
    H, r = Q.dense_case(rows, cols)
    R, rc = lv.compress_qr(gpu_ctx, H, r)
    assert R.shape == (cols, cols) and np.isfinite(R).all() and np.isfinite(rc).all()
    assert np.all(R[np.tril_indices(cols, -1)] == 0)
    Href, rref = Q.reference_dense(H, r)
    e, b = _errors(f"dense_{rows}x{cols}", H, r, R, rc, Href, rref)
    assert e.max() <= b, np.unravel_index(np.argmax(e), e.shape)


@pytest.mark.parametrize("rows,cols", [(1, 1), (16, 16), (40, 64), (64, 64), (5, 97)])
def test_compress_qr_leaves_short_matrices_alone(gpu_ctx, rows, cols):
    """rows <= cols: nothing to remove; rows_out = rows and the whole buffer comes back bit-unchanged"""
    from larvio_amd import larvio as lv
    H, r = Q.dense_case(rows, cols)
    ld = _filter_ld(cols)
    Hb, rb, k = lv.compress_qr(gpu_ctx, H, r, ld=ld)
    H0, r0 = lv._padded_qr(H, r, ld)
    assert k == rows and _same_bits(Hb, H0) and _same_bits(rb, r0)


def test_compress_qr_capacity(gpu_ctx):
    """65,537 rows: LVK_ERR_CAPACITY (3) before anything is launched (the buffers come back unchanged), and the same context then
    completes a normal call.  65,536 rows compute: test_compress_qr_dense_stage[65536-17]."""
    from larvio_amd import larvio as lv
    from larvio_amd._lib import _p
    rng = np.random.default_rng(65537)
    H = rng.normal(0, 1, (65537, 17)); r = rng.normal(0, 1, 65537)
    dH, dr = gpu_ctx.to_device(H), gpu_ctx.to_device(r)
    out = C.c_int(-1)
    st = lv._L().lvk_ekf_compress_qr(gpu_ctx.h, _p(dH), 17, 65537, 17, _p(dr), C.byref(out))
    assert st == 3 and out.value == -1
    assert _same_bits(gpu_ctx.to_host(dH, np.float64, H.shape), H) and _same_bits(gpu_ctx.to_host(dr, np.float64, r.shape), r)
    H2, r2 = Q.dense_case(700, 17)
    R, rc = lv.compress_qr(gpu_ctx, H2, r2)
    Href, rref = Q.reference_dense(H2, r2)
    e, b = _errors("dense_700x17_after_capacity_error", H2, r2, R, rc, Href, rref)
    assert e.max() <= b


# --------------------------------------------------------------------------------------------------- the filter's layout
@pytest.mark.parametrize("rows,cols", [(700, 40), (1044, 64), (543, 33), (98, 97), (9217, 48)])
def test_compress_qr_padded_ld(gpu_ctx, rows, cols):
    """lvk_ekf_compress_qr as the filter calls it (ld = ((cols + 15) & ~15) + 8, NaN in the padding columns and in two rows past the
    matrix, and past the rows of r): the same bits as the packed call, every byte of padding unchanged"""
    from larvio_amd import larvio as lv
    H, r = Q.dense_case(rows, cols)
    ld = _filter_ld(cols)
    R, rc = lv.compress_qr(gpu_ctx, H, r)
    Hb, rb, k = lv.compress_qr(gpu_ctx, H, r, ld=ld)
    H0, r0 = lv._padded_qr(H, r, ld)
    assert k == len(R)
    assert _same_bits(Hb[:k, :cols], R) and _same_bits(rb[:k], rc)
    assert _same_bits(Hb[:, cols:], H0[:, cols:]) and _same_bits(Hb[rows:], H0[rows:]) and _same_bits(rb[rows:], r0[rows:])


@pytest.mark.parametrize("name", ["mixed_rpl16", "mixed_rpl8", "burst_3_levels", "steady_copies", "lds_100x130", "lds_63x257", "reg_63x256"])
def test_compress_qr_groups_padded_ld(gpu_ctx, name):
    """lvk_ekf_compress_qr_groups as the filter calls it (layout as test_compress_qr_padded_ld): the same bits as the packed call,
    every byte of padding unchanged"""
    from larvio_amd import larvio as lv
    c = Q.group_case(name)
    H, r = c["H"], c["r"]
    rows, cols = H.shape
    ld = _filter_ld(cols)
    Hc, rc = lv.compress_qr_groups(gpu_ctx, H, r, c["groups"])
    Hb, rb, k = lv.compress_qr_groups(gpu_ctx, H, r, c["groups"], ld=ld)
    H0, r0 = lv._padded_qr(H, r, ld)
    assert k == len(Hc)
    assert _same_bits(Hb[:k, :cols], Hc) and _same_bits(rb[:k], rc)
    assert _same_bits(Hb[:, cols:], H0[:, cols:]) and _same_bits(Hb[rows:], H0[rows:]) and _same_bits(rb[rows:], r0[rows:])


# --------------------------------------------------------------------------------------------------- negligible columns
@pytest.mark.parametrize("kernel", Q.NEGLIGIBLE_KERNELS)
@pytest.mark.parametrize("side", ["below", "above"])
def test_negligible_column(gpu_ctx, kernel, side):
    """QR_NEGLIGIBLE (sum of squares <= 1e-200: the column is left alone) in the register, LDS and dense reflector kernels.  Below: one
    column of entries ~1e-110 - finite output, every pair without that column within the bound, pairs with it within 2 c_i c_j (what
    dropping the column's remainder can cost).  Above: entries ~1e-95 (sum of squares ~1e-188) - processed like any other column,
    every pair within the bound."""
    from larvio_amd import larvio as lv
    H, r, k, groups, N = Q.negligible_case(kernel, side)
    if groups is None:
        Hc, rc = lv.compress_qr(gpu_ctx, H, r)
        Href, rref = Q.reference_dense(H, r)
    else:
        levels, _ = lv.qr_plan(N, groups)
        Hc, rc = lv.compress_qr_groups(gpu_ctx, H, r, groups)
        Href, rref = Q.emulate(levels, H, r)
    assert np.isfinite(Hc).all() and np.isfinite(rc).all()
    e, b = _errors(f"negligible_{kernel}_{side}", H, r, Hc, rc, Href, rref)
    if side == "below":
        with_k = np.zeros(e.shape, bool); with_k[k, :] = True; with_k[:, k] = True
        print(f"QRSTAGE negligible_{kernel}_{side}: pairs without column {k}: kernel {e[~with_k].max():.3e}; with it: {e[with_k].max():.3e}")
        assert e[~with_k].max() <= b
        assert e[with_k].max() <= 2.0
    else:
        assert e.max() <= b
