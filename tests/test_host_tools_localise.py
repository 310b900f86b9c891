"""lvk::LarVio::localiseMap (include/lvk_larvio.hpp): tests/host/localise_check.cpp is compiled with g++ against the headers, linked with the
in-tree liblvk_hip.so and run.  It touches no device: the member's signature is checked by the compiler, the records' layout against
larvio_amd/_lib.py, and a call on handles that were never initialised is refused."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_localise_map_compiles_links_and_refuses_without_handles(tmp_path):
    from larvio_amd import ops
    from larvio_amd._lib import LOCALISE_INFO, MAP_OBS_INFO, LOCALISE_QUEUED, LOCALISE_NO_CLONE
    exe = str(tmp_path / "localise_check")
    lib_dir = os.path.join(ROOT, "larvio_amd")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "localise_check.cpp"),
                        "-L" + lib_dir, "-llvk_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "localiseMap 0"
    w = lines[1].split()
    got = dict(zip(w[0::2], (int(x) for x in w[1::2])))
    want = {k: LOCALISE_INFO.fields[k][1] for k in ("status", "n_ok", "n_bad", "clone_id", "map", "R_wc", "p_wc", "cov_cam")}
    want["sizeof"] = LOCALISE_INFO.itemsize
    assert got == want
    assert lines[2] == f"obs_info {MAP_OBS_INFO.itemsize} camera_pose_job {ops.CAMERA_POSE_JOB.itemsize} codes {LOCALISE_QUEUED} {LOCALISE_NO_CLONE}"
