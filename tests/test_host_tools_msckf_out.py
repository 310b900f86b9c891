"""examples/larvio_euroc --msckf-out: the option and the line format through examples/host_tools (no GPU), and the driver itself on the
synthetic ASL directory (GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "examples", "host_tools")


@pytest.fixture(scope="module")
def host_tools():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "examples"), "host_tools"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return TOOL


def _args(*a):
    r = subprocess.run([TOOL, "euroc-args", *a], capture_output=True, text=True)
    return r.returncode, dict(l.partition(" ")[::2] for l in r.stdout.splitlines()), r.stderr


def test_msckf_out_option_is_parsed_next_to_the_others(host_tools):
    rc, o, _ = _args()
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", max_frames="-1", pipelined="0")
    rc, o, _ = _args("--msckf-out", "points.txt")
    assert rc == 0 and o["msckf_out"] == "points.txt" and o["map_out"] == ""
    rc, o, _ = _args("--map-out", "m.txt", "--pipelined", "--msckf-out", "p.txt", "--max-frames", "12", "--tum", "t.txt", "--mask", "k.png")
    assert rc == 0 and o == dict(tum="t.txt", mask="k.png", map_out="m.txt", msckf_out="p.txt", max_frames="12", pipelined="1")
    rc, _, err = _args("--msckf-out")                                    # the file name is missing
    assert rc == 1 and "unknown option --msckf-out" in err
    rc, _, err = _args("--msckf")
    assert rc == 1 and "unknown option --msckf" in err


def _parse(line):
    w = line.split()
    assert len(w) == 14
    return int(w[0]), np.array(w[1:4], float), np.array(w[4:13], float).reshape(3, 3), int(w[13])


def test_msckf_out_line_round_trips_the_doubles(host_tools):
    rng = np.random.default_rng(3)
    A = rng.normal(0, 1, (3, 3)); S = A @ A.T * 1e-3; p = rng.normal(0, 5, 3)
    vals = [repr(float(x)) for x in list(p) + list(S.ravel())]
    r = subprocess.run([TOOL, "msckf-line", "123456789012", *vals, "17"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    i, pp, SS, n = _parse(lines[0])
    assert i == 123456789012 and n == 17 and np.array_equal(pp, p) and np.array_equal(SS, S)


@pytest.mark.gpu
def test_driver_writes_msckf_points_on_the_synthetic_directory(gpu_ctx, tmp_path):
    from larvio_amd import synthetic as S
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import TUMVI_LIKE
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from make_euroc_dir import write_euroc_dir
    cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
    frames = synth_frames(0, 64, cam=cam)                                # the frames of test_cpp_dataset_driver_on_an_asl_directory (cached)
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
    bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
    out_dir = str(tmp_path / "logs") + "/"; os.makedirs(out_dir)
    d = str(tmp_path / "seq")
    write_euroc_dir(d, frames, imu_all, fcfg, bcfg, output_dir=out_dir)
    base = [os.path.join(ROOT, "examples", "larvio_euroc"), d + "/mav0/imu0/data.csv", d + "/mav0/cam0/data.csv", d + "/mav0/cam0/data", d + "/config.yaml"]
    out = str(tmp_path / "points.txt"); tum = str(tmp_path / "t.txt"); tum0 = str(tmp_path / "t0.txt")
    r = subprocess.run(base + ["--msckf-out", out, "--tum", tum], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(out).read().splitlines()
    assert len(lines) > 0
    for l in lines:
        i, p, Sg, n = _parse(l)
        assert np.isfinite(p).all() and np.array_equal(Sg, Sg.T) and n >= bcfg["least_observation_number"]
        np.linalg.cholesky(Sg)
    print("%d MSCKF points written" % len(lines))
    r0 = subprocess.run(base + ["--tum", tum0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and open(tum0).read() == open(tum).read()      # the trajectory does not notice the export
    out2 = str(tmp_path / "points_pipelined.txt")
    r2 = subprocess.run(base + ["--msckf-out", out2, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert open(out2).read() == open(out).read()                         # lvk_vio_pipe: the same points
