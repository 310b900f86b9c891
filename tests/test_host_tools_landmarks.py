"""examples/larvio_euroc --landmarks: the option, the line format and the batching by time through examples/host_tools (no GPU), and the
driver itself on the synthetic ASL directory (GPU): it is refused with --pipelined, and a file without a single observation leaves the
trajectory file as it is without the option."""
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


def _fields(names, *a):
    r = subprocess.run([TOOL, "euroc-args-fields", names, *a], capture_output=True, text=True)
    return r.returncode, dict(l.partition(" ")[::2] for l in r.stdout.splitlines()), r.stderr


def test_landmarks_option_is_parsed_next_to_the_others(host_tools):
    rc, o, _ = _fields("landmarks")
    assert rc == 0 and o["landmarks"] == ""
    rc, o, _ = _fields("landmarks,fixes,tum", "--tum", "t.txt", "--landmarks", "l.csv")
    assert rc == 0 and o["landmarks"] == "l.csv" and o["fixes"] == "" and o["tum"] == "t.txt"
    rc, _, err = _fields("landmarks", "--landmarks")                     # the file name is missing
    assert rc == 1 and "unknown option --landmarks" in err
    r = subprocess.run([TOOL, "euroc-args-all", "--landmarks", "l.csv"], capture_output=True, text=True)
    assert r.returncode == 0 and [l.split(" ")[0] for l in r.stdout.splitlines()] == ["tum", "mask", "map_out", "msckf_out", "keyframes_out", "max_frames", "pipelined"]


def test_lines_are_parsed_and_batched_by_time(host_tools, tmp_path):
    rng = np.random.default_rng(5)
    times = [1.25, 1.25, 1.25, 1.3, 1.35, 1.35, 1.25]                    # equal times that are not consecutive open a new batch
    rows = [np.concatenate([[t], rng.normal(0, 1, 7) * 10.0 ** rng.uniform(-4, 2, 7)]) for t in times]
    f = tmp_path / "lm.csv"
    with open(f, "w") as h:
        h.write("#time,px,py,pz,u,v,sigma,sigma_w\n")
        for k, v in enumerate(rows):
            if k == 4:
                h.write("\n1,2,3\nnot a line\n")                         # skipped: too few fields, no number
            n = 7 if k in (1, 5) else 8                                  # sigma_w is optional: 0 when absent
            h.write((", " if k == 2 else ",").join(repr(float(x)) for x in v[:n]) + ("\r\n" if k == 3 else "\n"))
    r = subprocess.run([TOOL, "landmark-batches", str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    heads = [l.split() for l in lines if l.startswith("batch")]
    assert [(int(h[1]), float(h[3]), int(h[5])) for h in heads] == [(0, 1.25, 3), (1, 1.3, 1), (2, 1.35, 2), (3, 1.25, 1)]
    got = np.array([l.split() for l in lines if not l.startswith("batch")], float)
    want = np.array(rows); want[[1, 5], 7] = 0.0
    assert np.array_equal(got, want)                                     # the doubles round-trip
    empty = tmp_path / "none.csv"
    open(empty, "w").write("#time,px,py,pz,u,v,sigma\n")
    r = subprocess.run([TOOL, "landmark-batches", str(empty)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == ""
    assert subprocess.run([TOOL, "landmark-batches", str(tmp_path / "missing.csv")], capture_output=True, text=True).returncode == 1


@pytest.mark.gpu
def test_driver_with_an_empty_file_writes_the_same_trajectory_and_refuses_pipelined(gpu_ctx, tmp_path):
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
    tum0 = str(tmp_path / "t0.txt"); tum1 = str(tmp_path / "t1.txt")
    r0 = subprocess.run(base + ["--tum", tum0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "landmarks batches" not in r0.stdout and len(np.loadtxt(tum0)) >= 20
    empty = str(tmp_path / "none.csv")
    open(empty, "w").write("#time,px,py,pz,u,v,sigma,sigma_w\n")
    r1 = subprocess.run(base + ["--tum", tum1, "--landmarks", empty], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert open(tum1).read() == open(tum0).read() and "landmarks batches 0 refused 0 queued 0 applied 0" in r1.stdout
    rp = subprocess.run(base + ["--landmarks", empty, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert rp.returncode == 1 and "--landmarks is not available with --pipelined" in rp.stderr
