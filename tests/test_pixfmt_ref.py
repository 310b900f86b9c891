"""CPU: the pixel-format definitions of include/lvk_c.h as tests/pixfmt_ref.py restates them, the Python marshalling of the formats,
and the kernel's per-lane routines (larvio_amd/csrc/fe_pixfmt_dev.h) run on the host under AddressSanitizer / UBSan by the
stand-alone harness tests/host/pixfmt_check.hip."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pixfmt_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_and_codes_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "lvk_c.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define LVK_PIX_([A-Z0-9]+)\s+(\d+)", txt)}
    assert codes == PR.CODE
    assert "(1868*B + 9617*G + 4899*R + 8192) >> 14" in txt          # the header states the formula: it is the contract
    from larvio_amd._lib import PIX_FORMATS, pixfmt_bytes_per_pixel
    assert PIX_FORMATS == PR.CODE
    assert {f: pixfmt_bytes_per_pixel(f) for f in PR.FORMATS} == PR.BPP


def test_grey_triples_map_to_themselves():
    g = np.arange(256)
    assert np.array_equal(PR.gray_from_bgr(g, g, g), g)
    assert 1868 + 9617 + 4899 == 1 << 14


def test_colour_formula_stays_in_range_over_all_triples_and_is_monotone():
    v = np.arange(256, dtype=np.int32)
    lo, hi = 255, 0
    for r in range(256):                                     # 256 planes of 65,536 triples = all 2^24
        plane = PR.gray_from_bgr(v[:, None], v[None, :], r)
        lo = min(lo, int(plane.min())); hi = max(hi, int(plane.max()))
        assert (np.diff(plane, axis=0) >= 0).all() and (np.diff(plane, axis=1) >= 0).all()      # in B and in G
        if r:
            assert (plane >= prev).all()                     # in R
        prev = plane
    assert (lo, hi) == (0, 255)


def test_colour_layouts_pick_the_right_bytes():
    px = np.array([[[10, 100, 200, 77]]], np.uint8)
    want_bgr = (1868 * 10 + 9617 * 100 + 4899 * 200 + 8192) >> 14
    want_rgb = (1868 * 200 + 9617 * 100 + 4899 * 10 + 8192) >> 14
    assert want_bgr != want_rgb
    assert PR.to_gray(px[..., :3], "bgr8")[0, 0] == want_bgr and PR.to_gray(px, "bgra8")[0, 0] == want_bgr
    assert PR.to_gray(px[..., :3], "rgb8")[0, 0] == want_rgb and PR.to_gray(px, "rgba8")[0, 0] == want_rgb
    px2 = px.copy(); px2[..., 3] = 200                       # alpha is ignored
    assert PR.to_gray(px2, "bgra8")[0, 0] == want_bgr and PR.to_gray(px2, "rgba8")[0, 0] == want_rgb


def test_mono16_edge_values_at_every_shift():
    v = np.array([[0, 0xFF, 0x100, 0xFFFF]], np.uint16)
    want = {0: [0, 255, 255, 255], 1: [0, 127, 128, 255], 2: [0, 63, 64, 255], 3: [0, 31, 32, 255], 4: [0, 15, 16, 255],
            5: [0, 7, 8, 255], 6: [0, 3, 4, 255], 7: [0, 1, 2, 255], 8: [0, 0, 1, 255]}
    for shift in range(9):
        assert PR.to_gray(v, "mono16", shift).tolist() == [want[shift]], shift
    with pytest.raises(AssertionError):
        PR.to_gray(v, "mono16", 9)


def test_yuv_layouts_pick_the_right_bytes():
    stream = np.array([[16, 128, 17, 129, 18, 130, 19, 131]], np.uint8)       # as YUYV: Y = 16 17 18 19; as UYVY: Y = 128 129 130 131
    img = stream.reshape(1, 4, 2)
    assert PR.to_gray(img, "yuyv").tolist() == [[16, 17, 18, 19]]
    assert PR.to_gray(img, "uyvy").tolist() == [[128, 129, 130, 131]]


def test_from_gray_builds_frames_that_are_not_grey():
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (6, 8), dtype=np.uint8)
    for fmt in PR.FORMATS[1:]:
        shift = 4 if fmt == "mono16" else 0
        img = PR.from_gray(rng, g, fmt, shift)
        assert img.shape[:2] == g.shape and img.view(np.uint8).size == g.size * PR.BPP[fmt]
        back = PR.to_gray(img, fmt, shift)
        if fmt in ("mono16", "yuyv", "uyvy"):
            assert np.array_equal(back, g)
        else:
            assert np.abs(back.astype(int) - g).max() <= 40 and not np.array_equal(img[..., 0], img[..., 1])


def test_python_marshalling_accepts_what_the_format_demands_and_names_both_otherwise():
    from larvio_amd._lib import make_image, pixfmt_host_array
    h, w = 6, 10
    good = {"bgr8": np.zeros((h, w, 3), np.uint8), "rgba8": np.zeros((h, w, 4), np.uint8), "mono16": np.zeros((h, w), np.uint16),
            "yuyv": np.zeros((h, w, 2), np.uint8)}
    for fmt, a in good.items():
        im, keep = make_image(a, fmt=fmt)
        assert (im.width, im.height, im.stride, im.is_device) == (w, h, w * PR.BPP[fmt], 0) and keep is a
    wide = np.zeros((h, w + 3, 3), np.uint8)[:, 1:1 + w]                    # a window of a wider image: rows keep their stride
    im, keep = make_image(wide, fmt="bgr8")
    assert im.stride == 3 * (w + 3) and im.data == wide.ctypes.data
    assert pixfmt_host_array(np.zeros((h, w, 3), np.uint8)[:, ::2], "bgr8").flags.c_contiguous      # strided pixels are packed
    for fmt, a in (("bgr8", np.zeros((h, w), np.uint8)), ("bgr8", np.zeros((h, w, 4), np.uint8)), ("mono16", np.zeros((h, w), np.uint8)),
                   ("yuyv", np.zeros((h, w, 3), np.uint8)), ("rgba8", np.zeros((h, w, 4), np.float32))):
        with pytest.raises(ValueError) as e:
            make_image(a, fmt=fmt)
        assert fmt in str(e.value) and str(a.shape) in str(e.value) and a.dtype.name in str(e.value)
    im, _ = make_image(device_ptr=4096, shape=(h, w), fmt="bgra8")
    assert im.stride == 4 * w and im.is_device == 1
    im, keep = make_image(np.zeros((h, w), np.uint8))                       # the default is untouched
    assert im.stride == w


def test_lane_routines_on_the_host_under_asan_and_ubsan(tmp_path):
    """tests/host/pixfmt_check.hip: every source row in a heap block of exactly w * bytes_per_pixel bytes, the destination row in one of
    exactly w bytes, every format, w = 1..9, 63, 64, 65, source and destination offsets 0..3 - a read or write past a row is a
    sanitizer report, a wrong byte a mismatch against the harness's own plain loop."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "pixfmt_check")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "larvio_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", "pixfmt_check.hip"), "-o", exe, "-fsanitize=address,undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"pixfmt_check: (\d+) rows, (\d+) vectorised lanes, 0 mismatches", r.stdout)
    assert m and int(m.group(1)) >= 8 * 12 * 4 and int(m.group(2)) > 0, r.stdout
