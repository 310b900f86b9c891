"""The selection half of cv::goodFeaturesToTrack restated in plain numpy / Python, from a float32 response map, and the counters
of the two selection kernels (k_gftt_candidates, k_gftt_select in larvio_amd/csrc/fe_image.hip) restated next to it.

select() is the rule tests/test_oracle_frontend.py::test_good_features_vs_python_greedy_selection spells out, with the part of
the behaviour that test leaves out: the grid of rint(minDistance) cells and its 3x3 cell neighbourhood, as OpenCV, the oracle and
the kernel have it (only corners in the nine cells around a candidate are tested).  tests/test_gftt_ref.py holds it to the oracle,
and to the rule without a grid: on integer pixels the grid hides no conflict.

The counters do not compute corners: the GPU stage tests use them to prove, before touching the GPU, that a hand-made map reaches
the branch of the kernels it is named for."""
import numpy as np

# ---- the kernels' constants (fe_image.hip)
GC_COLS, GC_ROWS = 256, 8          # pixels one k_gftt_candidates workgroup scans
GC_LIST_BEFORE = 1024              # its local list before it was made to hold the whole tile (GC_COLS * GC_ROWS / 2)
GF_HIST_BITS = 13                  # strength histogram: top bits of the 32-bit order key (1/16 octave per bin)
GF_GROUP = 8                       # bins per group: buckets are whole groups on the fast path
GF_SURV = 8192                     # survivor buffer (keys), halved when the cell grid is fine
GF_MAX_OUT = 4096
LDS_BYTES = 160 * 1024
GF_STATIC_LDS = (36 * 1024, 40 * 1024)   # k_gftt_select's static LDS lies in between (histogram 32 KB + group sums 4 KB + a few words);
                                         # the host asks the runtime for the figure, surv_cap() refuses shapes where it would matter


def threshold(eig, quality, mask=None):
    """float32 threshold of goodFeaturesToTrack: (float)(masked maximum as double * quality); 0 when nothing is unmasked"""
    eig = np.asarray(eig, np.float32)
    valid = eig[mask != 0] if mask is not None else eig.ravel()
    mx = np.float64(valid.max()) if valid.size else np.float64(0.0)
    return np.float32(mx * np.float64(quality))


def candidates(eig, quality, mask=None):
    """-> (values float32, pixel indices int64) of the NMS candidates, in image order: THRESH_TOZERO at the threshold, non-zero,
    unmasked, equal to the 3x3 dilation of the thresholded map, not on the 1-pixel border"""
    eig = np.asarray(eig, np.float32)
    h, w = eig.shape
    thr = np.where(eig > threshold(eig, quality, mask), eig, np.float32(0))
    c = thr[1:h - 1, 1:w - 1]
    dil = c.copy()
    for dy in range(3):
        for dx in range(3):
            np.maximum(dil, thr[dy:dy + h - 2, dx:dx + w - 2], out=dil)
    cand = (c != 0) & (c == dil)
    if mask is not None:
        cand &= np.asarray(mask)[1:h - 1, 1:w - 1] != 0
    ys, xs = np.nonzero(cand)
    return c[ys, xs], (ys + 1).astype(np.int64) * w + (xs + 1)


def select(eig, max_corners, quality, min_distance, mask=None):
    """-> (n, 2) float32 corners (x, y) in the order goodFeaturesToTrack accepts them; max_corners <= 0: no limit"""
    eig = np.asarray(eig, np.float32)
    h, w = eig.shape
    vals, idx = candidates(eig, quality, mask)
    order = np.lexsort((idx, vals))[::-1]                    # strength descending, then pixel index descending
    cell = int(np.rint(min_distance))                        # rint: 20.5 -> 20, 7.5 -> 8
    md2 = float(np.float32(min_distance * min_distance))     # dx*dx + dy*dy is an exact small integer in float32
    grid, out = {}, []
    for k in idx[order].tolist():
        y, x = divmod(k, w)
        xc, yc = x // cell, y // cell
        good = True
        for yy in (yc - 1, yc, yc + 1):
            for xx in (xc - 1, xc, xc + 1):
                for ax, ay in grid.get((xx, yy), ()):
                    if (x - ax) * (x - ax) + (y - ay) * (y - ay) < md2:
                        good = False
                        break
                if not good:
                    break
            if not good:
                break
        if good:
            grid.setdefault((xc, yc), []).append((x, y))
            out.append((x, y))
            if max_corners > 0 and len(out) == max_corners:
                break
    return np.array(out, np.float32).reshape(-1, 2)


# ---------------------------------------------------------------- the kernels' counters
def order_key(vals):
    """f2ord: the 32-bit key whose unsigned order is the float order"""
    b = np.asarray(vals, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def tile_counts(idx, w, h):
    """candidates per k_gftt_candidates workgroup: (rows of tiles, columns of tiles); a tile is 256 columns x 8 rows from pixel (1, 1)"""
    idx = np.asarray(idx, np.int64)
    gx, gy = (w - 2 + GC_COLS - 1) // GC_COLS, (h - 2 + GC_ROWS - 1) // GC_ROWS
    out = np.zeros((gy, gx), np.int64)
    np.add.at(out, ((idx // w - 1) // GC_ROWS, (idx % w - 1) // GC_COLS), 1)
    return out


def bin_counts(vals):
    """candidates per histogram bin (8192 bins over the top 13 key bits) and per group of 8 bins"""
    bins = np.bincount(order_key(vals) >> np.uint32(32 - GF_HIST_BITS), minlength=1 << GF_HIST_BITS).astype(np.int64)
    return bins, bins.reshape(-1, GF_GROUP).sum(1)


def surv_cap(w, h, min_distance, max_corners):
    """size of k_gftt_select's survivor buffer for a shape as lvk_gftt_run chooses it: 8192, 4096 when the cell grid is fine,
    0 = refused (LVK_ERR_CAPACITY).  A shape whose answer depends on the exact static LDS of the kernel is an error of the test."""
    cell = int(np.rint(min_distance))
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell

    def rule(static):
        avail = LDS_BYTES - static
        for cap in (GF_SURV, GF_SURV // 2):
            if cap * 8 + gw * gh * 8 + max_corners * 4 <= avail:
                return cap
        return 0
    a, b = (rule(s) for s in GF_STATIC_LDS)
    if a != b:
        raise ValueError(f"{w}x{h} at min_distance {min_distance}, {max_corners} corners: too close to the LDS limit to name its branch")
    return a


def first_bucket(vals, max_corners):
    """k_gftt_select's first bucket on its group-aligned path -> (candidates in it, groups it spans): whole groups from the strongest
    down until they hold `target` candidates (64 doubled up to 4 * max_corners, at most 1024), or all there is"""
    target = 64
    while target < 4 * max_corners and target < 1024:
        target <<= 1
    _, groups = bin_counts(vals)
    nz = np.nonzero(groups)[0]
    if len(nz) == 0:
        return 0, 0
    suffix = np.cumsum(groups[::-1])[::-1]                   # candidates in groups [g, top]
    fit = np.nonzero(suffix >= target)[0]
    lo = fit[-1] if len(fit) else 0
    return int(suffix[lo]), int(np.count_nonzero(groups[lo:]))
