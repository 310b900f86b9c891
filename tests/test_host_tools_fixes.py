"""examples/larvio_euroc --fixes / --fix-max-gap: the options and the line format through examples/host_tools (no GPU), and the driver
itself on the synthetic ASL directory (GPU): fixes taken from the driver's own trajectory are all applied, and a file without a
single fix leaves the trajectory file as it is without the option."""
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


def test_fixes_options_are_parsed_next_to_the_others(host_tools):
    rc, o, _ = _fields("fixes,fix_max_gap")
    assert rc == 0 and o["fixes"] == "" and float(o["fix_max_gap"]) == 0.0
    rc, o, _ = _fields("fixes,fix_max_gap,tum,keyframes_out", "--tum", "t.txt", "--fixes", "f.csv", "--fix-max-gap", "0.25")
    assert rc == 0 and o["fixes"] == "f.csv" and float(o["fix_max_gap"]) == 0.25 and o["tum"] == "t.txt" and o["keyframes_out"] == ""
    rc, _, err = _fields("fixes", "--fixes")                             # the file name is missing
    assert rc == 1 and "unknown option --fixes" in err
    rc, _, err = _fields("fixes", "--fix-max-gap")
    assert rc == 1 and "unknown option --fix-max-gap" in err
    # the listings that have always been printed keep their lines
    r = subprocess.run([TOOL, "euroc-args-all", "--fixes", "f.csv"], capture_output=True, text=True)
    assert r.returncode == 0 and [l.split(" ")[0] for l in r.stdout.splitlines()] == ["tum", "mask", "map_out", "msckf_out", "keyframes_out", "max_frames", "pipelined"]


def _line(text):
    r = subprocess.run([TOOL, "fix-line", text], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip()


def test_fix_line_format(host_tools):
    rng = np.random.default_rng(3)
    v = rng.normal(0, 1, 14) * 10.0 ** rng.uniform(-6, 3, 14); v[1] = 1.0
    assert np.array_equal(np.array(_line(",".join(repr(float(x)) for x in v)).split(), float), v)                     # the doubles round-trip
    short = np.array(_line(", ".join(repr(float(x)) for x in v[:11]) + "\r\n").split(), float)                        # no lever arm: zeros
    assert np.array_equal(short[:11], v[:11]) and np.all(short[11:] == 0)
    for bad in ("#time,kind,px,py,pz,qx,qy,qz,qw,sigma_p,sigma_theta", "", "1,0,1,2,3", "1,2,0,0,0,0,0,0,1,0.1,0.1", "1,0,0,0,0,0,0,0,1,0.1,0.1,0.5"):
        assert _line(bad) == "no fix", bad


@pytest.mark.gpu
def test_driver_applies_the_fixes_of_a_file_on_the_synthetic_directory(gpu_ctx, tmp_path):
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
    tum0 = str(tmp_path / "t0.txt"); tum1 = str(tmp_path / "t1.txt"); tum2 = str(tmp_path / "t2.txt")
    r0 = subprocess.run(base + ["--tum", tum0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert "fixes read" not in r0.stdout
    traj = np.loadtxt(tum0)
    assert len(traj) >= 20
    # a file without a single fix: the trajectory file is the one written without the option
    empty = str(tmp_path / "none.csv")
    open(empty, "w").write("#time,kind,px,py,pz,qx,qy,qz,qw,sigma_p,sigma_theta\n")
    r1 = subprocess.run(base + ["--tum", tum1, "--fixes", empty], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    assert open(tum1).read() == open(tum0).read() and "fixes read 0 refused 0 queued 0 applied 0" in r1.stdout
    # position fixes at the driver's own poses (state times to the nanosecond the file prints: equal to a clone's time or a rounding
    # away from it, which --fix-max-gap turns into an interpolation with a weight next to 0 or 1), every fourth pose, the last poses left
    # out so that none waits for a frame that never comes; a residual of millimetres against sigma 0.05 m passes the default gate
    rows = traj[4:-4:4]
    fx = str(tmp_path / "fixes.csv")
    with open(fx, "w") as f:
        f.write("#time,kind,px,py,pz,qx,qy,qz,qw,sigma_p,sigma_theta\n")
        for t in rows:
            f.write("%.9f,0,%.17g,%.17g,%.17g,0,0,0,1,0.05,0.01\n" % (t[0], t[1], t[2], t[3]))
    r2 = subprocess.run(base + ["--tum", tum2, "--fixes", fx, "--fix-max-gap", "0.2"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    last = [l for l in r2.stdout.splitlines() if l.startswith("fixes read")]
    print(last)
    assert len(last) == 1
    w = last[0].split(); st = dict(zip(w[1::2], map(int, w[2::2])))
    assert st["read"] == len(rows) and st["refused"] == 0 and st["queued"] == len(rows) and st["applied"] == len(rows), st
    assert st["gated"] == st["not_pd"] == st["stale"] == st["no_clone"] == st["waiting"] == 0
    assert len(np.loadtxt(tum2)) == len(traj)
    rp = subprocess.run(base + ["--fixes", fx, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert rp.returncode == 1 and "--pipelined" in rp.stderr
