"""Numpy restatement of the pixel-format definitions of include/lvk_c.h (lvk_image_to_gray), in integer arithmetic and written from
the header's text, not from the kernel: what the GPU conversion and the front-end fed a non-default format are compared against.

Arrays: colour (H, W, 3|4) uint8, mono16 (H, W) uint16, yuyv / uyvy (H, W, 2) uint8 - pixel x of a row owns the bytes [2x, 2x + 2) of
the 4:2:2 stream (Y0 U Y1 V ... / U Y0 V Y1 ...).  Every function returns (H, W) uint8."""
import numpy as np

FORMATS = ("mono8", "bgr8", "rgb8", "bgra8", "rgba8", "mono16", "yuyv", "uyvy")
CODE = {n: i for i, n in enumerate(FORMATS)}
BPP = dict(mono8=1, bgr8=3, rgb8=3, bgra8=4, rgba8=4, mono16=2, yuyv=2, uyvy=2)


def gray_from_bgr(b, g, r):
    """grey = (1868*B + 9617*G + 4899*R + 8192) >> 14, exact integers; NOT narrowed: the caller may look at the range"""
    b, g, r = (np.asarray(v).astype(np.int32) for v in (b, g, r))       # at most 16384 * 255 + 8192: far inside 32 bits
    return (1868 * b + 9617 * g + 4899 * r + 8192) >> 14


def gray_from_mono16(v, shift):
    assert 0 <= shift <= 8
    return np.minimum(255, np.asarray(v).astype(np.int32) >> shift)


def to_gray(img, fmt, shift=0):
    img = np.asarray(img)
    if fmt == "mono8":
        assert img.dtype == np.uint8 and img.ndim == 2
        return img.copy()
    if fmt in ("bgr8", "bgra8"):
        assert img.dtype == np.uint8 and img.shape[2] == BPP[fmt]
        return gray_from_bgr(img[..., 0], img[..., 1], img[..., 2]).astype(np.uint8)
    if fmt in ("rgb8", "rgba8"):
        assert img.dtype == np.uint8 and img.shape[2] == BPP[fmt]
        return gray_from_bgr(img[..., 2], img[..., 1], img[..., 0]).astype(np.uint8)
    if fmt == "mono16":
        assert img.dtype == np.uint16 and img.ndim == 2
        return gray_from_mono16(img, shift).astype(np.uint8)
    if fmt in ("yuyv", "uyvy"):
        assert img.dtype == np.uint8 and img.shape[2] == 2 and img.shape[1] % 2 == 0
        return img[..., 0 if fmt == "yuyv" else 1].copy()
    raise ValueError(fmt)


def random_image(rng, fmt, h, w):
    """an image of format `fmt` with every byte random"""
    if fmt == "mono8":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if fmt == "mono16":
        return rng.integers(0, 65536, (h, w), dtype=np.uint16)
    return rng.integers(0, 256, (h, w, BPP[fmt]), dtype=np.uint8)


def from_gray(rng, gray, fmt, shift=0):
    """an image of format `fmt` that is NOT grey but whose to_gray() is whatever it is: colour noise around a grey frame, so that a
    front-end fed it sees a realistic picture (the test compares against to_gray of the result, not against `gray`)"""
    g = np.asarray(gray, np.uint8)
    h, w = g.shape
    if fmt == "mono8":
        return g.copy()
    if fmt == "mono16":
        return ((g.astype(np.uint16) << shift) | rng.integers(0, 1 << shift, (h, w), dtype=np.uint16)).astype(np.uint16)
    if fmt in ("yuyv", "uyvy"):
        out = rng.integers(0, 256, (h, w, 2), dtype=np.uint8)
        out[..., 0 if fmt == "yuyv" else 1] = g
        return out
    out = np.empty((h, w, BPP[fmt]), np.uint8)
    for c in range(3):
        out[..., c] = np.clip(g.astype(np.int32) + rng.integers(-40, 41, (h, w)), 0, 255)
    if BPP[fmt] == 4:
        out[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    return out
