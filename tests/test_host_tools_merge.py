"""lvk::ImageProcessor::mergeMap (include/lvk_larvio.hpp): tests/host/merge_check.cpp is compiled with g++ against the headers, linked with
the in-tree liblvk_hip.so and run.  It touches no device: the member's signature is checked by the compiler, the 3D alignment's records'
layout against larvio_amd/_lib.py, lvk_align_invert against larvio_amd.localize.invert_alignment, and a call on a handle that was never
initialised is refused."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_map_compiles_links_and_refuses_without_a_handle(tmp_path):
    from larvio_amd import localize as L
    from larvio_amd._lib import ALIGN3D_MATCH, ALIGN3D_HYP, Align3dOptions
    exe = str(tmp_path / "merge_check")
    lib_dir = os.path.join(ROOT, "larvio_amd")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "merge_check.cpp"),
                        "-L" + lib_dir, "-llvk_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "mergeMap 0"
    w = lines[1].split()
    got = dict(zip(w[0::2], (int(x) for x in w[1::2])))
    want = dict(match=ALIGN3D_MATCH.itemsize, X=ALIGN3D_MATCH.fields["X"][1], Y=ALIGN3D_MATCH.fields["Y"][1], hyp=ALIGN3D_HYP.itemsize,
                options=C.sizeof(Align3dOptions), thresh=Align3dOptions.thresh.offset, min_rho=Align3dOptions.min_rho.offset, min_inliers=Align3dOptions.min_inliers.offset)
    want.update({k: ALIGN3D_HYP.fields[k][1] for k in ("n_models", "count", "c", "s", "t")})
    assert got == want
    c, s, t = L.invert_alignment(dict(c=0.6, s=0.8, t=[3.0, -2.0, 0.5]))
    w = lines[2].split()
    assert w[0] == "invert" and int(w[1]) == 0 and [float(x) for x in w[2:7]] == [c, s, *t]
    assert w[7:] == ["status", "0", "rms", "0", "null", "1"]
