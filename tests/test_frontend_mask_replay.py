"""CPU side of the region mask for corner detection (lvk_frontend_set_mask): the shadow replay that judges the masked GPU runs
(tests/mask_replay.py) is itself held to the oracle, every masked case is shown not to be vacuous on the oracle alone, and the
example driver's --mask refuses a mask of the wrong size before it touches a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mask_replay as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_UNMASKED = {}


def _oracle_run(name):
    """the unmasked oracle over a named stream, with the replay (all-255 user mask) checked after every frame;
    -> (configuration, [(kind, new points after the frame)])"""
    if name in _UNMASKED:
        return _UNMASKED[name]
    from oracle import lvo
    frames, seq, cfg = MR.sequence(name)
    ora = lvo.Frontend(cfg)
    rep = MR.Replay(cfg)
    full = np.full((cfg["height"], cfg["width"]), 255, np.uint8)
    out = []
    for ts, img in frames:
        imu = MR.imu_for(seq, ts)
        rep.before(ora)
        have, _ = ora.process(img, ts, imu)
        kind, want = rep.check(ora, img, have, full, imu["t"][0] if len(imu) else None, ts)
        out.append((kind, want))
    _UNMASKED[name] = (cfg, out)
    return _UNMASKED[name]


@pytest.mark.parametrize("name,min_frames", [("headline", 60), ("odd", 60)])
def test_replay_with_a_full_mask_is_the_oracle(name, min_frames):
    """byte for byte after EVERY frame (Replay.check asserts it): the bootstrap frames, every re-detection, and the frames between"""
    cfg, out = _oracle_run(name)
    kinds = [k for k, _ in out]
    assert len(out) >= min_frames
    assert kinds.count("bootstrap") >= 1 and kinds.count("redetect") >= 20 and kinds.count("idle") >= 10, kinds
    assert sum(len(p) for k, p in out if k == "redetect") >= 50          # the re-detections do find corners


def test_replay_with_no_mask_is_the_full_mask():
    """None and all-255 are the same detection (OpenCV's empty mask)"""
    frames, seq, cfg = MR.sequence("odd", 3)
    full = np.full((cfg["height"], cfg["width"]), 255, np.uint8)
    img = frames[0][1]
    a = MR.replay_bootstrap(cfg, img, None); b = MR.replay_bootstrap(cfg, img, full)
    assert len(a) > 20 and MR.same_bits(a, b)
    tr = a[::3]
    assert MR.same_bits(MR.replay_redetect(cfg, img, tr, None), MR.replay_redetect(cfg, img, tr, full))
    assert len(MR.replay_redetect(cfg, img, np.zeros((cfg["max_features_num"], 2), np.float32), None)) == 0      # no budget left


@pytest.mark.parametrize("case", [c[0] for c in MR.masked_cases()])
def test_masked_cases_are_not_vacuous(case):
    """the UNMASKED oracle puts at least 10 new corners where the case's mask forbids them: a product that ignored the mask
    could not pass the case's parity test"""
    _, name, build = next(c for c in MR.masked_cases() if c[0] == case)
    cfg, out = _oracle_run(name)
    mask = build(cfg["width"], cfg["height"])
    assert mask.shape == (cfg["height"], cfg["width"]) and mask.dtype == np.uint8
    assert (mask == 0).any() and (mask != 0).any()
    n = sum(MR.corners_in_forbidden_area(p, mask) for k, p in out if k != "idle")
    print(case, "unmasked corners inside the forbidden area:", n)
    assert n >= 10, n


def test_mask_builders():
    for h in (480, 203, 512):
        rows = MR.seam_rows(h)
        rem = {r % MR.MM_ROWS for r in rows}
        assert len(rows) >= 6 and rem == {MR.MM_ROWS - 1, 0, 1}, (h, rows)      # edges on k MM_ROWS - 1, k MM_ROWS, k MM_ROWS + 1
    hp = MR.half_plane_mask(752, 480)
    assert not hp[:, :376].any() and set(np.unique(hp[:, 376:]).tolist()) == {1, 7, 255}
    d = MR.disc_mask(512, 512, 250)
    assert d[256, 256] == 255 and d[0, 0] == 0 and d[256, 4] == 0 and d[256, 8] == 255
    b = MR.block_mask(301, 203)
    assert b.shape == (203, 301) and 0.3 < (b != 0).mean() < 0.8
    src = open(os.path.join(ROOT, "larvio_amd", "csrc", "fe_image.hip")).read()
    assert "#define MM_ROWS %d\n" % MR.MM_ROWS in src


def test_keep_out_mask_rounds_half_away_from_zero():
    cfg = dict(width=64, height=48, min_distance=3)
    m = MR.keep_out_mask(cfg, [[10.5, 20.5], [-0.5, 47.6], [63.49, 0.0]])
    want = np.full((48, 64), 255, np.uint8)
    want[18:25, 8:15] = 0          # round(10.5) = 11, round(20.5) = 21
    want[45:48, 0:3] = 0           # round(-0.5) = -1 -> columns -4..2 clipped; round(47.6) = 48 -> rows 45..51 clipped
    want[0:4, 60:64] = 0
    assert np.array_equal(m, want)


def test_dataset_driver_rejects_a_mask_of_the_wrong_size(tmp_path):
    """examples/larvio_euroc --mask: a PNG whose size is not the configured resolution is an error message and a non-zero exit,
    decided on the host before any device is asked for (the same run with a mask of the right size gets as far as the device)"""
    from PIL import Image
    from larvio_amd import synthetic as S
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from make_euroc_dir import write_euroc_dir
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "larvio_euroc"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "examples", "larvio_euroc")
    seq = S.imu_only_sequence()
    frames = [(seq.frame_time(i), np.zeros((480, 752), np.uint8)) for i in range(2)]
    d = str(tmp_path / "d")
    write_euroc_dir(d, frames, seq.imu_array(0, 30), S.frontend_config(), S.backend_config())
    args = [exe, d + "/mav0/imu0/data.csv", d + "/mav0/cam0/data.csv", d + "/mav0/cam0/data", d + "/config.yaml"]
    bad = str(tmp_path / "bad.png"); Image.fromarray(MR.disc_mask(512, 512, 250)).save(bad)
    r = subprocess.run(args + ["--mask", bad], capture_output=True, text=True)
    assert r.returncode == 1 and "the mask is 512x512, the configuration says 752x480" in r.stderr, r.stderr
    r = subprocess.run(args + ["--mask", str(tmp_path / "missing.png")], capture_output=True, text=True)
    assert r.returncode == 1 and "missing.png" in r.stderr, r.stderr
    r = subprocess.run(args + ["--mask"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown option" in r.stderr
    good = str(tmp_path / "good.png"); Image.fromarray(MR.disc_mask(752, 480, 230)).save(good)
    r = subprocess.run(args + ["--mask", good], capture_output=True, text=True)
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 3 and "no usable gfx950 device" in r.stderr, r.stderr


def test_mask_entry_points_are_bound():
    """the C ABI exports both calls and the Python class offers them (without a device there is nothing to call them on)"""
    import larvio_amd
    from larvio_amd._lib import lib
    L = lib()
    assert L.lvk_frontend_set_mask.restype is not None and L.lvk_frontend_has_mask.argtypes is not None
    assert callable(larvio_amd.ImageProcessor.set_mask) and isinstance(larvio_amd.ImageProcessor.has_mask, property)
    assert L.lvk_frontend_set_mask(None, None) != 0 and L.lvk_frontend_has_mask(None) == 0      # a null handle is refused, not dereferenced
