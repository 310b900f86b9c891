"""GPU stage tests of corner selection (k_gftt_candidates, k_gftt_select) on hand-made response maps, through the stage entry
lvk_good_features_from_map.  The judge is tests/gftt_ref.py (held to the oracle on the CPU by tests/test_gftt_ref.py): the corner
list must be identical, order included, in every case.  Each case first proves with the restated kernel counters - before it touches
the GPU - that its map reaches the branch it is named for; a case that does not is an error, not a skip."""
import ctypes as C
import numpy as np
import pytest

from tests import gftt_ref as R

pytestmark = pytest.mark.gpu

LVK_ERR_ARG, LVK_ERR_CAPACITY, LVK_ERR_UNSUPPORTED = 1, 3, 4


def gpu_select(ctx, eig, max_corners, md, mask=None, quality=0.01, cap=None, odd_mask_address=False):
    from larvio_amd import ops
    from larvio_amd._lib import lib, _p
    if not odd_mask_address:
        return ops.good_features_from_map(ctx, eig, max_corners, quality, md, mask, cap)
    eig = np.ascontiguousarray(eig, np.float32); h, w = eig.shape
    cap = max_corners if cap is None else cap
    buf = ctx.to_device(np.concatenate([np.zeros(1, np.uint8), np.ascontiguousarray(mask, np.uint8).ravel()]))
    d_eig = ctx.to_device(eig); d_out = ctx.alloc(8 * cap); d_n = ctx.alloc(4)
    ctx.check(lib().lvk_good_features_from_map(ctx.h, _p(d_eig), C.c_void_p(buf.ptr + 1), w, h, max_corners, quality, md, _p(d_out), cap, _p(d_n)))
    n = int(ctx.to_host(d_n, np.int32, (1,))[0])
    return ctx.to_host(d_out, np.float32, (cap, 2))[:n].copy()


def check(ctx, eig, max_corners, md, mask=None, quality=0.01, cap=None, what="", **kw):
    """the comparison every case ends in; -> the corner list"""
    want = R.select(eig, max_corners, quality, md, mask)
    if cap is not None:
        want = want[:cap]
    got = gpu_select(ctx, eig, max_corners, md, mask, quality, cap, **kw)
    print(f"{what} {eig.shape[1]}x{eig.shape[0]} md {md} max {max_corners}: reference {len(want)} corners, kernel {len(got)}")
    assert got.shape == want.shape and np.array_equal(got, want), (what, eig.shape, md, max_corners, len(got), len(want))
    return got


def lattice_map(w, h, values, rng=None, count=None):
    """`values` (an array, or a function of the number of sites) on the even-even interior lattice, 0 elsewhere: every site is a candidate"""
    ys, xs = np.mgrid[2:h - 1:2, 2:w - 1:2]
    ys, xs = ys.ravel(), xs.ravel()
    if count is not None:
        pick = rng.permutation(len(ys))[:count]
        ys, xs = ys[pick], xs[pick]
    eig = np.zeros((h, w), np.float32)
    eig[ys, xs] = values(len(ys)) if callable(values) else values
    return eig


def distinct_in(lo, hi, n, rng):
    """n distinct float32 values in [lo, hi), lo a power of two and hi <= 2 lo: distinct mantissas"""
    span = int((hi - lo) / lo * (1 << 23))
    return (np.float32(lo) * (1 + rng.choice(span, n, replace=False).astype(np.float64) / (1 << 23))).astype(np.float32)


def counters(eig, md, max_corners, mask=None):
    vals, idx = R.candidates(eig, 0.01, mask)
    h, w = eig.shape
    bins, groups = R.bin_counts(vals)
    return dict(n=len(vals), tile=int(R.tile_counts(idx, w, h).max()), bin=int(bins.max()), group=int(groups.max()),
                bins_used=int(np.count_nonzero(bins)), surv=R.surv_cap(w, h, md, max_corners), vals=vals)


# ---------------------------------------------------------------- the candidate kernel's local list
@pytest.mark.parametrize("md", [1.0, 3.0, 10.0])
def test_tile_overflow_on_a_plateau(gpu_ctx, md):
    eig = np.ones((20, 300), np.float32)
    c = counters(eig, md, 4096)
    assert c["n"] == 5364 and c["tile"] == 2048 > R.GC_LIST_BEFORE, c["tile"]       # fullest tile 2048 > 1024
    got = check(gpu_ctx, eig, 4096, md, what="plateau")
    assert len(got) > 20


# ---------------------------------------------------------------- one histogram bin over the survivor buffer
_ONE_BIN = {}


def one_bin_map(w):
    if w not in _ONE_BIN:
        rng = np.random.default_rng(w)
        _ONE_BIN[w] = lattice_map(w, w, lambda n: distinct_in(1.0, 1.03, n, rng))
    return _ONE_BIN[w]


@pytest.mark.parametrize("max_corners", [50, 1000, 4096])
@pytest.mark.parametrize("w,md,surv", [(200, 5.0, 8192), (180, 2.0, 4096)])
def test_one_bin_over_the_survivor_buffer(gpu_ctx, w, md, surv, max_corners):
    eig = one_bin_map(w)
    c = counters(eig, md, max_corners)
    assert c["surv"] == surv and c["bins_used"] == 1 and c["bin"] == c["n"] > surv, (c["bin"], c["surv"])   # 9801 > 8192; 7921 > 4096
    assert c["n"] == (9801 if w == 200 else 7921) and c["tile"] <= R.GC_LIST_BEFORE
    if w == 180:
        assert c["n"] < R.GF_SURV                              # only the halved buffer overflows
    got = check(gpu_ctx, eig, max_corners, md, what="one bin")
    assert len(got) == min(max_corners, len(R.select(eig, 0, 0.01, md)))


@pytest.mark.parametrize("levels", [1, 3])
def test_identical_strengths_order_by_pixel_index(gpu_ctx, levels):
    rng = np.random.default_rng(3)
    pick = np.array([1.0, 1.01, 1.02], np.float32)[:levels]
    eig = lattice_map(200, 200, lambda n: pick[rng.integers(0, levels, n)])
    c = counters(eig, 5.0, 1000)
    assert c["bins_used"] == 1 and c["bin"] == 9801 > c["surv"] == 8192 and len(np.unique(c["vals"])) == levels
    got = check(gpu_ctx, eig, 1000, 5.0, what=f"{levels} strengths")
    if levels == 1:
        k = got[:, 1] * 200 + got[:, 0]
        assert np.all(np.diff(k) < 0)                          # strictly descending pixel index
    assert R.surv_cap(200, 200, 2.0, 1000) == 4096             # 100 x 100 cells: the halved buffer
    check(gpu_ctx, eig, 1000, 2.0, what=f"{levels} strengths, fine grid")


def test_serial_walk_over_the_bins_of_one_group(gpu_ctx):
    rng = np.random.default_rng(5)
    eig = lattice_map(200, 200, lambda n: distinct_in(1.0, 1.5, n, rng))                # [1, 1.5): the 8 bins of one group
    for max_corners, md in ((1000, 5.0), (4096, 3.0), (30, 5.0)):
        c = counters(eig, md, max_corners)
        assert c["bins_used"] == 8 and c["bin"] <= c["surv"] == 8192 < c["group"] == 9801, (c["bin"], c["group"])
        check(gpu_ctx, eig, max_corners, md, what="serial walk")


# ---------------------------------------------------------------- the bitonic sort
def test_bitonic_sort_with_a_count_that_is_no_power_of_two(gpu_ctx):
    rng = np.random.default_rng(6)
    eig = lattice_map(320, 240, lambda n: distinct_in(1.0, 1.5, n, rng), rng, 700)
    vals, _ = R.candidates(eig, 0.01)
    assert R.first_bucket(vals, 1024)[0] == 700 > 512                                   # more than the rank sort takes; pads to 1024
    check(gpu_ctx, eig, 1024, 3.0, what="bitonic 700")
    # 3000 strong sites in one group, 2500 weak ones in a group far below: the first bucket is the 3000 (pads to 4096), the second is
    # mostly ruled out by the corners the first one gave
    ys, xs = np.mgrid[2:239:2, 2:319:2]
    site = rng.permutation(ys.size)[:5500]
    eig = np.zeros((240, 320), np.float32)
    eig[ys.ravel()[site[:3000]], xs.ravel()[site[:3000]]] = distinct_in(8.0, 12.0, 3000, rng)
    eig[ys.ravel()[site[3000:]], xs.ravel()[site[3000:]]] = distinct_in(1.0, 1.5, 2500, rng)
    vals, _ = R.candidates(eig, 0.01)
    assert len(vals) == 5500 and R.first_bucket(vals, 4096) == (3000, 1)
    got = check(gpu_ctx, eig, 4096, 3.0, what="bitonic 3000 + second bucket")
    weak = int((eig[got[:, 1].astype(int), got[:, 0].astype(int)] < 2).sum())
    assert 0 < weak < 2500 // 2, weak                                                   # the second bucket gives some, loses most


# ---------------------------------------------------------------- thresholds and signs
def test_threshold_edge_and_signs(gpu_ctx):
    # a maximum for which quality 0.01 taken through a float would move the threshold by an ulp (the kernel once did)
    q32 = np.float64(np.float32(0.01))
    mx = next(m for m in (np.float32(100) + np.arange(1, 200, dtype=np.float32) / 16)
              if np.float32(np.float64(m) * 0.01) > np.float32(np.float64(m) * q32))
    thr = np.float32(np.float64(mx) * 0.01)
    eig = np.zeros((40, 70), np.float32)
    eig[5, 5] = mx
    eig[20, 30] = thr                                         # exactly quality * max: out
    eig[30, 50] = np.nextafter(thr, np.float32(1e9))          # one ulp above: in
    assert R.threshold(eig, 0.01) == thr
    got = check(gpu_ctx, eig, 10, 3.0, what="threshold")
    assert np.array_equal(got, [[5, 5], [50, 30]])
    # slightly negative responses under a positive maximum
    rng = np.random.default_rng(7)
    eig = (rng.random((40, 70)) * 3).astype(np.float32)
    eig[rng.random((40, 70)) < 0.3] = np.float32(-1e-12)
    assert R.threshold(eig, 0.01) > 0 and (eig < 0).sum() > 500
    check(gpu_ctx, eig, 4096, 2.0, what="negative responses")
    mask = (rng.random((40, 70)) < 0.5).astype(np.uint8) * 3
    check(gpu_ctx, eig, 4096, 2.0, mask, what="negative responses, masked")
    # nothing to find
    zero = np.zeros((40, 70), np.float32)
    assert len(check(gpu_ctx, zero, 100, 3.0, what="all zero")) == 0
    assert len(check(gpu_ctx, eig, 100, 3.0, np.zeros((40, 70), np.uint8), what="all masked")) == 0
    border = np.zeros((40, 70), np.float32)
    border[0, :] = border[-1, :] = 5; border[:, 0] = border[:, -1] = 5
    border[1, 1:-1] = border[-2, 1:-1] = 1; border[1:-1, 1] = border[1:-1, -2] = 1     # interior, but each next to a larger border value
    assert len(check(gpu_ctx, border, 100, 3.0, what="maxima on the border only")) == 0


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize("w", [257, 258, 259, 513])
def test_tile_grid_edges(gpu_ctx, w):
    """257: the last interior column (255) still in the first column of workgroups; 258 / 259: the second column gets its first pixels;
    3 rows: one interior row; 10 / 11 and 18 rows: h - 2 = 8, 9 and 16 - a full tile row, one row more, two full ones"""
    rng = np.random.default_rng(w)
    for h in (3, 10, 11, 18):
        noise = rng.random((h, w)).astype(np.float32)
        steps = rng.integers(0, 5, (h, w)).astype(np.float32)                           # plateaus and ties
        mask = (rng.random((h, w)) < 0.7).astype(np.uint8) * 255
        gx, gy = (w - 2 + 255) // 256, (h - 2 + 7) // 8
        for eig in (noise, steps):
            eig[1:h - 1:2, w - 2] = 7 + np.arange(len(range(1, h - 1, 2)))                # corners in the last interior column and row
            eig[h - 2, 5] = 9
            _, idx = R.candidates(eig, 0.01)
            t = R.tile_counts(idx, w, h)
            assert t.shape == (gy, gx) and (w == 257 or t[:, -1].sum() > 0) and t[-1].sum() > 0, (w, h, t)   # the last tiles have work
            for md, maxc in ((1.0, 4096), (7.5, 4096), (20.5, 1)):
                check(gpu_ctx, eig, maxc, md, what="geometry")
            check(gpu_ctx, eig, 4096, 1.0, mask, what="geometry, mask at an odd address", odd_mask_address=True)
            check(gpu_ctx, eig, 300, 7.5, mask, what="geometry, masked")
    assert w % 4 != 0


def test_output_list_shorter_than_the_corners_found(gpu_ctx):
    rng = np.random.default_rng(9)
    eig = rng.random((60, 90)).astype(np.float32)
    assert len(R.select(eig, 500, 0.01, 2.0)) > 100
    got = check(gpu_ctx, eig, 500, 2.0, cap=10, what="cap 10")
    assert len(got) == 10                                      # n_out == cap
    assert len(check(gpu_ctx, eig, 1, 2.0, what="one corner")) == 1


# ---------------------------------------------------------------- state left behind
def test_twice_in_a_row_then_an_ordinary_image(gpu_ctx):
    """the selection kernel leaves the scratch words zeroed for the next detection; an overflowing map must not leak into the next call"""
    from tests.test_gftt_ref import oracle_map
    plateau = np.ones((20, 300), np.float32)
    assert counters(plateau, 3.0, 4096)["tile"] == 2048
    dense = one_bin_map(200)
    assert counters(dense, 5.0, 1000)["bin"] == 9801
    for _ in range(2):
        check(gpu_ctx, plateau, 4096, 3.0, what="plateau again")
        check(gpu_ctx, dense, 1000, 5.0, what="one bin again")
    p, eig = oracle_map("textured")
    got = check(gpu_ctx, eig, 200, 10.0, what="ordinary image")
    assert len(got) > 50 and np.array_equal(got, p.good_features(200, 0.01, 10.0))
    p, eig = oracle_map("checker4")                            # a regular target through the stage entry, against the oracle itself
    got = check(gpu_ctx, eig, 500, 10.0, what="checkerboard")
    assert len(got) > 50 and np.array_equal(got, p.good_features(500, 0.01, 10.0))


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_context_usable(gpu_ctx):
    from larvio_amd._lib import lib, _p
    L = lib()
    d_eig = gpu_ctx.to_device(np.ones((1000, 1000), np.float32))
    d_out = gpu_ctx.alloc(8 * 4096); d_n = gpu_ctx.alloc(4)

    def call(eig=d_eig, w=64, h=48, maxc=100, md=5.0, out=d_out, cap=100, n=d_n, ctx=gpu_ctx.h):
        return L.lvk_good_features_from_map(ctx, _p(eig), None, w, h, maxc, 0.01, md, _p(out), cap, _p(n))
    assert call(w=2) == LVK_ERR_ARG and call(h=2) == LVK_ERR_ARG and call(w=0) == LVK_ERR_ARG and call(h=-5) == LVK_ERR_ARG
    assert call(eig=None) == LVK_ERR_ARG and call(out=None) == LVK_ERR_ARG and call(n=None) == LVK_ERR_ARG and call(cap=-1) == LVK_ERR_ARG
    assert call(ctx=None) == LVK_ERR_ARG
    assert call(maxc=0) == LVK_ERR_UNSUPPORTED and call(maxc=-3) == LVK_ERR_UNSUPPORTED and call(maxc=4097) == LVK_ERR_UNSUPPORTED
    assert call(w=65536, h=65536) == LVK_ERR_ARG and call(w=46341, h=46341) == LVK_ERR_ARG          # w * h beyond 2^31 - 1
    assert call(md=0.99) == LVK_ERR_UNSUPPORTED and call(md=0.0) == LVK_ERR_UNSUPPORTED
    assert call(md=float("nan")) == LVK_ERR_UNSUPPORTED and call(md=float("inf")) == LVK_ERR_UNSUPPORTED and call(md=32768.0) == LVK_ERR_UNSUPPORTED
    assert b"minDistance" in L.lvk_last_error(gpu_ctx.h)
    assert R.surv_cap(1000, 1000, 2.0, 100) == 0               # 500 x 500 cells of 8 bytes: no room in LDS
    assert call(w=1000, h=1000, md=2.0) == LVK_ERR_CAPACITY
    assert b"LDS" in L.lvk_last_error(gpu_ctx.h)
    assert call(w=3, h=3, maxc=4096, md=1.0, cap=4096) == 0    # the smallest map there is: one interior pixel
    gpu_ctx.sync()
    assert int(gpu_ctx.to_host(d_n, np.int32, (1,))[0]) == 1
    rng = np.random.default_rng(10)
    check(gpu_ctx, rng.random((48, 64)).astype(np.float32), 100, 5.0, what="after the refusals")


# ---------------------------------------------------------------- the frame path
def test_frame_path_on_a_checkerboard(gpu_ctx):
    """lvk_frontend_process on a 320 x 240 checkerboard of 4 px squares, no CLAHE, against the oracle's front-end frame by frame (the
    comparison of tests/test_gpu_frontend_edge.py: state, tracks, descriptors, new corners, message).  The first frame detects with the
    plain route; the later frames take the mask-and-maximum kernel and the prepared scratch words, which the stage entry does not reach.
    Every candidate of this image lies in one histogram bin."""
    from oracle import lvo
    from tests.test_gftt_ref import checker
    from tests.test_gpu_frontend_edge import _cfg, _run
    img = checker(4)
    cfg = _cfg(320, 240, max_features_num=200, min_distance=20, pyramid_levels=2, flag_equalize=0)
    c = counters(lvo.LkPyramid(img, 21, 0).min_eigen_map(), 20.0, 200)
    assert c["bin"] > c["surv"] == 8192, c["bin"]
    new = []
    _run(gpu_ctx, [img, img, img], cfg, on_frame=lambda i, have, msg, state, tracks, pts: new.append(len(pts)))
    assert new[0] > 50, new
