"""examples/larvio_euroc --keyframes-out: the option and the line format through examples/host_tools (no GPU), and the driver itself on
the synthetic ASL directory (GPU)."""
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


def _args(*a, cmd="euroc-args-all"):
    r = subprocess.run([TOOL, cmd, *a], capture_output=True, text=True)
    return r.returncode, dict(l.partition(" ")[::2] for l in r.stdout.splitlines()), r.stderr


def test_keyframes_out_option_is_parsed_next_to_the_others(host_tools):
    rc, o, _ = _args()
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", keyframes_out="", max_frames="-1", pipelined="0")
    rc, o, _ = _args("--keyframes-out", "kf.txt")
    assert rc == 0 and o["keyframes_out"] == "kf.txt" and o["msckf_out"] == "" and o["map_out"] == ""
    rc, o, _ = _args("--map-out", "m.txt", "--keyframes-out", "k.txt", "--pipelined", "--msckf-out", "p.txt", "--max-frames", "12", "--tum", "t.txt", "--mask", "k.png")
    assert rc == 0 and o == dict(tum="t.txt", mask="k.png", map_out="m.txt", msckf_out="p.txt", keyframes_out="k.txt", max_frames="12", pipelined="1")
    rc, _, err = _args("--keyframes-out")                                # the file name is missing
    assert rc == 1 and "unknown option --keyframes-out" in err
    rc, _, err = _args("--keyframes")
    assert rc == 1 and "unknown option --keyframes" in err
    # euroc-args accepts the option and keeps the six lines it has always printed
    rc, o, _ = _args("--keyframes-out", "kf.txt", cmd="euroc-args")
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", max_frames="-1", pipelined="0")


def _parse(line):
    w = line.split()
    assert len(w) == 90
    v = np.array(w[2:], float)
    return dict(id=int(w[0]), to_id=int(w[1]), time=v[0], to_time=v[1], q=v[2:6], p=v[6:9], rel_q=v[9:13], rel_p=v[13:16], cov_abs=v[16:52].reshape(6, 6),
                cov_rel=v[52:88].reshape(6, 6), all=v)


def test_keyframes_out_line_round_trips_the_doubles(host_tools):
    rng = np.random.default_rng(4)
    v = rng.normal(0, 1, 88) * 10.0 ** rng.uniform(-9, 3, 88)
    r = subprocess.run([TOOL, "keyframe-line", "123456789012", "123456789019", *[repr(float(x)) for x in v]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    k = _parse(lines[0])
    assert k["id"] == 123456789012 and k["to_id"] == 123456789019 and np.array_equal(k["all"], v)


@pytest.mark.gpu
def test_driver_writes_keyframes_on_the_synthetic_directory(gpu_ctx, tmp_path):
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
    out = str(tmp_path / "kf.txt"); tum = str(tmp_path / "t.txt"); tum0 = str(tmp_path / "t0.txt")
    r = subprocess.run(base + ["--keyframes-out", out, "--tum", tum], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(out).read().splitlines()
    assert len(lines) > 0
    ids = []
    for l in lines:
        k = _parse(l)
        assert np.isfinite(k["all"]).all() and k["to_id"] > k["id"] and k["to_time"] > k["time"]
        assert abs(np.linalg.norm(k["q"]) - 1) < 1e-9 and abs(np.linalg.norm(k["rel_q"]) - 1) < 1e-9
        for Sg in (k["cov_abs"], k["cov_rel"]):
            assert np.array_equal(Sg, Sg.T) and np.linalg.eigvalsh(Sg).min() >= -1e-12 * np.trace(Sg)
        ids.append(k["id"])
    assert len(set(ids)) == len(ids)
    print("%d keyframes written" % len(lines))
    r0 = subprocess.run(base + ["--tum", tum0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and open(tum0).read() == open(tum).read()      # the trajectory does not notice the export
    out2 = str(tmp_path / "kf_pipelined.txt")
    r2 = subprocess.run(base + ["--keyframes-out", out2, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert open(out2).read() == open(out).read()                         # lvk_vio_pipe: the same records
