"""GPU: lvk_image_to_gray, the stage entry behind the front-end's input pixel formats (include/lvk_c.h states the formulas).

Every comparison is array_equal against tests/pixfmt_ref.py, the numpy restatement of the header's text.  Source rows sit at every
byte alignment and with padded strides inside a larger allocation, the destination lies in a plane of sentinel bytes that must survive
wherever the contract does not write: the padding of each row and the rows beyond h."""
import ctypes as C

import numpy as np
import pytest

from tests import pixfmt_ref as PR

pytestmark = pytest.mark.gpu

LVK_OK, LVK_ERR_ARG = 0, 1
SENTINEL = 0xA5
WIDTHS = (1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257)
HEIGHTS = (1, 2, 3)


class _Bench:
    """one source and one destination device buffer reused by every call of a test"""

    def __init__(self, ctx, src_bytes, dst_bytes):
        from larvio_amd._lib import lib
        self.ctx, self.L = ctx, lib()
        self.src = ctx.alloc(src_bytes); self.dst = ctx.alloc(dst_bytes)

    def convert(self, raw, base, sstride, w, h, fmt, shift, dstride, extra_rows=2, dst_base=0):
        """raw: (h, w * bpp) uint8 rows.  -> (status, whole destination plane of h + extra_rows rows as uint8 (rows, dstride))"""
        L, ctx = self.L, self.ctx
        host = np.random.default_rng(w * 131 + h).integers(0, 256, base + h * sstride, dtype=np.uint8)      # junk around the rows
        for y in range(h):
            host[base + y * sstride: base + y * sstride + raw.shape[1]] = raw[y]
        n_dst = (h + extra_rows) * dstride
        assert host.nbytes <= self.src.nbytes and dst_base + n_dst <= self.dst.nbytes
        ctx.check(L.lvk_memcpy_h2d(ctx.h, C.c_void_p(self.src.ptr), host.ctypes.data_as(C.c_void_p), host.nbytes))
        ctx.check(L.lvk_memset(ctx.h, C.c_void_p(self.dst.ptr), SENTINEL, dst_base + n_dst))
        st = L.lvk_image_to_gray(ctx.h, C.c_void_p(self.src.ptr + base), sstride, w, h, PR.CODE[fmt], shift, C.c_void_p(self.dst.ptr + dst_base), dstride)
        out = ctx.to_host(self.dst.ptr + dst_base, np.uint8, (h + extra_rows, dstride))
        return st, out

    def free(self):
        self.src.free(); self.dst.free()


def _raw(img, h):
    return np.ascontiguousarray(img).view(np.uint8).reshape(h, -1)


def _check_plane(out, want, w, h, tag):
    assert np.array_equal(out[:h, :w], want), tag
    assert (out[:h, w:] == SENTINEL).all(), ("padding overwritten", tag)
    assert (out[h:] == SENTINEL).all(), ("rows beyond h overwritten", tag)


@pytest.mark.parametrize("fmt", PR.FORMATS)
def test_every_format_at_every_alignment_and_stride(gpu_ctx, fmt):
    bpp = PR.BPP[fmt]
    two = fmt == "mono16"
    rng = np.random.default_rng(PR.CODE[fmt] + 1)
    bench = _Bench(gpu_ctx, 4 + 3 * (257 * bpp + 14) + 64, 8 + 5 * (257 + 5))
    n = 0
    for w in WIDTHS:
        if fmt in ("yuyv", "uyvy") and w % 2:
            continue
        for h in HEIGHTS:
            img = PR.random_image(rng, fmt, h, w)
            shift = int(rng.integers(0, 9)) if two else 0
            want = PR.to_gray(img, fmt, shift)
            raw = _raw(img, h)
            for pad in ((0, 2, 14) if two else (0, 1, 13)):
                for base in ((0, 2) if two else (0, 1, 2, 3)):
                    for dpad in (0, 5):
                        st, out = bench.convert(raw, base, w * bpp + pad, w, h, fmt, shift, w + dpad)
                        assert st == LVK_OK, gpu_ctx.check(st)
                        _check_plane(out, want, w, h, (fmt, w, h, pad, base, dpad, shift))
                        n += 1
    # the destination's own base alignment (the front-end's plane is aligned; a caller's need not be)
    w, h = 65, 3
    if fmt in ("yuyv", "uyvy"):
        w = 66
    img = PR.random_image(rng, fmt, h, w); want = PR.to_gray(img, fmt, 0)
    for dst_base in (1, 2, 3):
        st, out = bench.convert(_raw(img, h), 0, w * bpp, w, h, fmt, 0, w + 5, dst_base=dst_base)
        assert st == LVK_OK
        _check_plane(out, want, w, h, (fmt, "dst_base", dst_base))
    bench.free()
    assert n >= 6 * 3 * 3 * 2 * 2


def test_every_colour_triple_once_as_bgr8_and_as_rgb8(gpu_ctx):
    """4096 x 4096 pixels = all 2^24 (byte0, byte1, byte2) triples; the same bytes read as BGR8 and as RGB8"""
    from larvio_amd import ops
    idx = np.arange(1 << 24, dtype=np.uint32)
    img = np.empty((4096, 4096, 3), np.uint8)
    flat = img.reshape(-1, 3)
    flat[:, 0] = idx & 255; flat[:, 1] = (idx >> 8) & 255; flat[:, 2] = idx >> 16
    del idx
    for fmt in ("bgr8", "rgb8"):
        got = ops.image_to_gray(gpu_ctx, img, fmt)
        want = PR.to_gray(img, fmt)
        assert np.array_equal(got, want), fmt


def test_every_mono16_value_at_every_shift(gpu_ctx):
    from larvio_amd import ops
    img = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    for shift in range(9):
        got = ops.image_to_gray(gpu_ctx, img, "mono16", shift)
        assert np.array_equal(got, PR.to_gray(img, "mono16", shift)), shift
    assert got[255, 255] == 255 and got[0, 255] == 0            # shift 8: 0xFFFF -> 255, 0x00FF -> 0


def test_the_same_bits_twice(gpu_ctx):
    from larvio_amd import ops
    rng = np.random.default_rng(7)
    for fmt in PR.FORMATS:
        img = PR.random_image(rng, fmt, 203, 302)
        a = ops.image_to_gray(gpu_ctx, img, fmt); b = ops.image_to_gray(gpu_ctx, img, fmt)
        assert np.array_equal(a, b) and np.array_equal(a, PR.to_gray(img, fmt)), fmt


def test_refusals_leave_the_context_usable(gpu_ctx):
    from larvio_amd._lib import lib
    L = lib()
    rng = np.random.default_rng(3)
    w, h = 64, 4
    bench = _Bench(gpu_ctx, 4096, 4096)
    src, dst = bench.src.ptr, bench.dst.ptr
    code = PR.CODE

    def call(s=src, ss=None, ww=w, hh=h, fmt="bgr8", shift=0, d=dst, ds=None):
        c = fmt if isinstance(fmt, int) else code[fmt]
        bpp = PR.BPP.get(fmt, 1) if not isinstance(fmt, int) else 1
        return L.lvk_image_to_gray(gpu_ctx.h, C.c_void_p(s) if s else None, ww * bpp if ss is None else ss, ww, hh, c, shift,
                                   C.c_void_p(d) if d else None, ww if ds is None else ds)

    bad = {
        "null source": call(s=None), "null destination": call(d=None),
        "w = 0": call(ww=0, ss=192, ds=64), "w < 0": call(ww=-4, ss=192, ds=64), "h = 0": call(hh=0), "h < 0": call(hh=-1),
        "format -1": call(fmt=-1, ss=256), "format 8": call(fmt=8, ss=256),
        "source stride too small": call(ss=3 * w - 1), "mono8 stride too small": call(fmt="mono8", ss=w - 1),
        "destination stride too small": call(ds=w - 1),
        "shift -1": call(fmt="mono16", shift=-1), "shift 9": call(fmt="mono16", shift=9),
        "shift with bgr8": call(shift=1), "shift with mono8": call(fmt="mono8", shift=4), "shift with yuyv": call(fmt="yuyv", shift=8),
        "odd w yuyv": call(fmt="yuyv", ww=63), "odd w uyvy": call(fmt="uyvy", ww=63),
        "odd stride mono16": call(fmt="mono16", ss=2 * w + 1), "odd base mono16": call(fmt="mono16", s=src + 1),
    }
    assert all(v == LVK_ERR_ARG for v in bad.values()), {k: v for k, v in bad.items() if v != LVK_ERR_ARG}
    assert L.lvk_image_to_gray(None, C.c_void_p(src), 3 * w, w, h, 1, 0, C.c_void_p(dst), w) == LVK_ERR_ARG
    assert b"mono16" in L.lvk_last_error(gpu_ctx.h)
    # and one good call on the same context
    img = PR.random_image(rng, "bgr8", h, w)
    st, out = bench.convert(_raw(img, h), 0, 3 * w, w, h, "bgr8", 0, w)
    assert st == LVK_OK
    _check_plane(out, PR.to_gray(img, "bgr8"), w, h, "after the refusals")
    bench.free()
