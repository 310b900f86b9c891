"""tests/gftt_ref.py held to the CPU oracle (no GPU): the numpy restatement of goodFeaturesToTrack's selection equals
lvo_good_features on the oracle's own response maps - a textured image and three regular ones, where equal strengths abound and
the order comes from the pixel index - and the restated kernel counters count what they say."""
import os
import re
import numpy as np
import pytest
from oracle import lvo
from tests import gftt_ref as R

W, H = 320, 240


def textured(w=W, h=H, seed=4):
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    a = rng.uniform(0, 255, (h // 4 + 2, w // 4 + 2))
    return np.clip(ndimage.zoom(a, 4, order=3)[:h, :w] + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def checker(square, w=W, h=H, lo=20, hi=220):
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // square) + (y // square)) & 1, hi, lo).astype(np.uint8)


def dots(w=W, h=H, pitch=6, lo=20, hi=220):
    """2 x 2 dots on a `pitch` px lattice"""
    y, x = np.mgrid[0:h, 0:w]
    return np.where((x % pitch < 2) & (y % pitch < 2), hi, lo).astype(np.uint8)


IMAGES = {"textured": textured, "checker4": lambda: checker(4), "checker2": lambda: checker(2), "dots": dots}
_MAPS = {}


def oracle_map(name):
    """(oracle pyramid, its min-eigenvalue map) of a named image, computed once"""
    if name not in _MAPS:
        p = lvo.LkPyramid(IMAGES[name](), 21, 0)
        _MAPS[name] = (p, p.min_eigen_map())
    return _MAPS[name]


def region_mask(w=W, h=H):
    m = np.full((h, w), 255, np.uint8)
    m[:, : w // 3] = 0
    m[h // 2:h // 2 + 30, :] = 0
    m[5::7, 3::5] = 0                  # isolated holes: a masked pixel still suppresses its neighbours
    m[h - 40:, w - 50:] = 1            # any non-zero byte allows
    return m


@pytest.mark.parametrize("md", [1.0, 7.5, 10.0, 20.5])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", list(IMAGES))
def test_restatement_equals_oracle(name, masked, md):
    p, eig = oracle_map(name)
    mask = region_mask() if masked else None
    for maxc in (4096, 37):
        want = p.good_features(maxc, 0.01, md, mask)
        got = R.select(eig, maxc, 0.01, md, mask)
        assert got.shape == want.shape and np.array_equal(got, want), (name, masked, md, maxc, len(got), len(want))
    assert len(want) == 37


def test_regular_images_are_full_of_ties():
    """what makes the three regular images a test of the tie rule: most candidates share their strength with another one"""
    for name in ("checker4", "checker2", "dots"):
        vals, _ = R.candidates(oracle_map(name)[1], 0.01)
        assert len(vals) > 1000 and len(np.unique(vals)) < len(vals) // 10, (name, len(vals), len(np.unique(vals)))


def test_cell_grid_against_the_all_pairs_rule():
    """The grid of rint(minDistance) cells with its 3x3 neighbourhood is restated as OpenCV has it.  On integer pixels it hides no
    conflict: minDistance <= cell + 0.5, and two pixels two cells apart are at least cell + 1 apart.  So the restatement must equal the
    rule without a grid (every accepted corner tested), also where minDistance is not an integer and rint goes either way."""
    rng = np.random.default_rng(8)
    eig = np.zeros((90, 130), np.float32)
    ys, xs = rng.integers(0, 90, 500), rng.integers(0, 130, 500)
    eig[ys, xs] = rng.integers(1, 40, 500).astype(np.float32)          # few distinct strengths: ties by pixel index
    for md in (1.0, 2.5, 7.5, 8.49, 20.5):
        vals, idx = R.candidates(eig, 0.01)
        acc = []
        for k in idx[np.lexsort((idx, vals))[::-1]].tolist():
            y, x = divmod(k, 130)
            if all(np.float32((x - ax) ** 2 + (y - ay) ** 2) >= np.float32(md * md) for ax, ay in acc):
                acc.append((x, y))
        got = R.select(eig, 0, 0.01, md)
        assert len(acc) > 5 and np.array_equal(got, np.array(acc, np.float32)), md


def test_threshold_mask_and_border_rules():
    eig = np.zeros((8, 9), np.float32)
    eig[3, 3] = 100.0
    thr = np.float32(np.float64(np.float32(100.0)) * 0.01)
    assert R.threshold(eig, 0.01) == thr
    eig[5, 6] = thr                                        # exactly at the threshold: out (THRESH_TOZERO keeps v > thresh)
    assert np.array_equal(R.select(eig, 10, 0.01, 1.0), [[3, 3]])
    eig[5, 6] = np.nextafter(thr, np.float32(2))
    assert np.array_equal(R.select(eig, 10, 0.01, 1.0), [[3, 3], [6, 5]])
    eig[0, 4] = eig[7, 2] = eig[4, 0] = eig[2, 8] = 50.0   # border rows and columns are never corners, but they do suppress
    eig[1, 4] = 40.0
    assert np.array_equal(R.select(eig, 10, 0.01, 1.0), [[3, 3], [6, 5]])
    mask = np.full(eig.shape, 7, np.uint8); mask[3, 3] = 0  # the maximum is masked: the threshold follows the unmasked maximum (50)
    assert R.threshold(eig, 0.01, mask) == np.float32(0.5)
    assert np.array_equal(R.select(eig, 10, 0.01, 1.0, mask), [[6, 5]])
    assert len(R.select(eig, 10, 0.01, 1.0, np.zeros(eig.shape, np.uint8))) == 0
    assert len(R.select(np.zeros((5, 5), np.float32), 10, 0.01, 1.0)) == 0
    tie = np.zeros((6, 12), np.float32); tie[2, 2] = tie[2, 9] = tie[4, 5] = 1.0
    assert np.array_equal(R.select(tie, 2, 0.01, 2.0), [[5, 4], [9, 2]])     # equal strength: larger pixel index first


def test_counters_on_hand_made_maps():
    eig = np.ones((20, 300), np.float32)                   # a plateau: every interior pixel is its own 3x3 maximum
    vals, idx = R.candidates(eig, 0.01)
    assert len(vals) == 298 * 18
    assert np.array_equal(R.tile_counts(idx, 300, 20), [[2048, 336], [2048, 336], [512, 84]])
    bins, groups = R.bin_counts(vals)
    assert bins.sum() == len(vals) and bins[0xBF800000 >> 19] == len(vals) and groups[(0xBF800000 >> 19) // 8] == len(vals)
    b, g = R.bin_counts(np.array([1.0, 1.0624999, 1.0625, 1.99, 2.0, 0.5, -1e-12], np.float32))
    k1 = 0xBF800000 >> 19
    assert b[k1] == 2 and b[k1 + 1] == 1 and b[k1 + 15] == 1 and b[k1 + 16] == 1 and b[k1 - 16] == 1
    assert b[: 1 << 12].sum() == 1                         # negative strengths sort below every positive one
    assert g[k1 // 8] == 3 and g.sum() == 7
    assert list(R.order_key(np.array([-2.0, -1e-12, 0.0, 1e-12, 2.0], np.float32))) == sorted(R.order_key(np.array([-2.0, -1e-12, 0.0, 1e-12, 2.0], np.float32)))
    # tiles start at pixel (1, 1): column 256 is the last of the first tile, row 9 the first of the second
    assert np.array_equal(R.tile_counts([1 * 600 + 256, 1 * 600 + 257, 9 * 600 + 1, 8 * 600 + 598], 600, 12), [[1, 1, 1], [1, 0, 0]])


def test_surv_cap_rule():
    assert R.surv_cap(752, 480, 20.0, 4096) == 8192
    assert R.surv_cap(752, 480, 6.0, 600) == 4096          # 126 x 80 cells: the fine grid
    assert R.surv_cap(200, 200, 5.0, 4096) == 8192
    assert R.surv_cap(180, 180, 2.0, 4096) == 4096
    assert R.surv_cap(1000, 1000, 2.0, 100) == 0           # LVK_ERR_CAPACITY
    assert R.surv_cap(320, 240, 7.5, 100) == R.surv_cap(320, 240, 8.0, 100) == 8192
    with pytest.raises(ValueError):
        R.surv_cap(752, 480, 6.0, 3000)                    # fits or not by a few hundred bytes of the kernel's static LDS


def test_first_bucket():
    v = np.concatenate([np.full(700, 8.0), np.full(5000, 1.0)]).astype(np.float32)
    assert R.first_bucket(v[:700], 1024) == (700, 1)       # fewer than the target: all there is
    assert R.first_bucket(v, 1024) == (5700, 2)            # 700 < 1024: the next group down comes with it
    assert R.first_bucket(v, 10) == (700, 1)               # target 64
    assert R.first_bucket(v[:0], 10) == (0, 0)


def test_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "larvio_amd", "csrc", "fe_image.hip")).read()

    def define(name):
        return int(re.search(r"^#define %s (\d+)" % name, src, re.M).group(1))
    got = tuple(define(n) for n in ("GC_COLS", "GC_ROWS", "GF_HIST_BITS", "GF_SURV", "GF_MAX_OUT"))
    assert got == (R.GC_COLS, R.GC_ROWS, R.GF_HIST_BITS, R.GF_SURV, R.GF_MAX_OUT)
    assert R.GF_GROUP == (1 << R.GF_HIST_BITS) // 1024
