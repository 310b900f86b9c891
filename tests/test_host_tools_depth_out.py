"""examples/larvio_euroc --depth-out: the option and the line format through examples/host_tools (no GPU), and the driver itself on
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


ALL = "tum,mask,map_out,msckf_out,keyframes_out,depth_out,max_frames,pipelined"


def _args(*a, cmd="euroc-args-fields", fields=ALL):
    r = subprocess.run([TOOL, cmd] + ([fields] if cmd == "euroc-args-fields" else []) + list(a), capture_output=True, text=True)
    return r.returncode, dict(l.partition(" ")[::2] for l in r.stdout.splitlines()), r.stderr


def test_depth_out_option_is_parsed_next_to_the_others(host_tools):
    rc, o, _ = _args()
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", keyframes_out="", depth_out="", max_frames="-1", pipelined="0")
    rc, o, _ = _args("--depth-out", "d.txt")
    assert rc == 0 and o["depth_out"] == "d.txt" and o["keyframes_out"] == "" and o["msckf_out"] == "" and o["map_out"] == ""
    rc, o, _ = _args("--map-out", "m.txt", "--depth-out", "d.txt", "--keyframes-out", "k.txt", "--pipelined", "--msckf-out", "p.txt", "--max-frames", "12", "--tum", "t.txt",
                     "--mask", "k.png")
    assert rc == 0 and o == dict(tum="t.txt", mask="k.png", map_out="m.txt", msckf_out="p.txt", keyframes_out="k.txt", depth_out="d.txt", max_frames="12", pipelined="1")
    rc, _, err = _args("--depth-out")                                    # the file name is missing
    assert rc == 1 and "unknown option --depth-out" in err
    rc, _, err = _args("--depth")
    assert rc == 1 and "unknown option --depth" in err
    rc, o, _ = _args("--depth-out", "d.txt", "--pipelined", fields="pipelined,depth_out")      # the fields asked for, in that order
    assert rc == 0 and list(o.items()) == [("pipelined", "1"), ("depth_out", "d.txt")]
    rc, _, err = _args(fields="depth_out,nonsense")
    assert rc == 2 and "unknown field nonsense" in err
    # the older listings accept the option and keep the lines they have always printed
    rc, o, _ = _args("--depth-out", "d.txt", cmd="euroc-args-all")
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", keyframes_out="", max_frames="-1", pipelined="0")
    rc, o, _ = _args("--depth-out", "d.txt", cmd="euroc-args")
    assert rc == 0 and o == dict(tum="", mask="", map_out="", msckf_out="", max_frames="-1", pipelined="0")


def _parse(line):
    w = line.split()
    assert len(w) == 11
    v = np.array(w[2:], float)
    S = np.array([[v[3], v[4], v[5]], [v[4], v[6], v[7]], [v[5], v[7], v[8]]])
    return dict(stamp=w[0], t=float(w[0]), id=int(w[1]), p=v[:3], S=S, all=v)


def test_depth_out_line_round_trips_the_doubles(host_tools):
    rng = np.random.default_rng(5)
    p = rng.normal(0, 1, 3) * 10.0 ** rng.uniform(-3, 2, 3)
    c = rng.normal(0, 1, 9) * 10.0 ** rng.uniform(-9, 1, 9)
    r = subprocess.run([TOOL, "depth-line", "1403636580.5", "123456789012", *[repr(float(x)) for x in np.concatenate([p, c])]], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    k = _parse(lines[0])
    assert k["stamp"] == "1403636580.500000000" and k["id"] == 123456789012
    assert np.array_equal(k["p"], p) and np.array_equal(k["all"][3:], c[[0, 1, 2, 4, 5, 8]])


@pytest.mark.gpu
def test_driver_writes_one_line_per_feature_per_pose_on_the_synthetic_directory(gpu_ctx, tmp_path):
    """150 frames from rest (static initialiser, zero-velocity updates, then motion: the filter admits features into its state five
    seconds after the last zero-velocity update).  The file must hold, pose by pose and in the getter's order, exactly what the Python
    mirror of the loop gets from LarVio.get_features_in_camera() after each update - ids, positions and the six upper entries of Sigma,
    double for double - under the stamp of that pose; the --pipelined run (the getter inside the filter thread's odometry callback)
    must write the same file, the adapter's LarVio::getFeaturesInCamera (adapter_main --depth-out) the same lines but for the stamp;
    the trajectory does not notice the option."""
    import larvio_amd
    from larvio_amd import synthetic as S
    from larvio_amd.vio import VioDriver
    from tests.conftest import synth_frames
    from tests.test_gpu_vio_driver import TUMVI_LIKE
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "-s"])
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "adapter"), "-s"])
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from make_euroc_dir import write_euroc_dir
    cam = dict(TUMVI_LIKE); cam["T_cam_imu"] = S.EUROC["T_cam_imu"]
    frames = synth_frames(0, 150, cam=cam)
    seq = S.imu_only_sequence(cam=cam)
    ts = [f[0] for f in frames]
    imu_all = seq.imu_array(max(int(ts[0] * 200) - 4, 0), int(ts[-1] * 200) + 40)
    fcfg = S.frontend_config(cam=cam, max_features_num=300, min_distance=15)
    bcfg = S.backend_config(cam=cam, sw_size=12, if_zupt_valid=1)
    out_dir = str(tmp_path / "logs") + "/"; os.makedirs(out_dir)
    d = str(tmp_path / "seq")
    t_img, t_imu = write_euroc_dir(d, frames, imu_all, fcfg, bcfg, output_dir=out_dir)
    args = [d + "/mav0/imu0/data.csv", d + "/mav0/cam0/data.csv", d + "/mav0/cam0/data", d + "/config.yaml"]
    base = [os.path.join(ROOT, "examples", "larvio_euroc")] + args
    out = str(tmp_path / "depth.txt"); tum = str(tmp_path / "t.txt"); tum0 = str(tmp_path / "t0.txt")
    r = subprocess.run(base + ["--depth-out", out, "--tum", tum], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(out).read().splitlines()
    assert len(lines) > 0
    poses = [l.split()[0] for l in open(tum).read().splitlines()]
    per_pose = {}
    for l in lines:
        k = _parse(l)
        assert k["stamp"] in poses                                        # written after a pose, with that pose's stamp
        per_pose.setdefault(k["stamp"], []).append(k)
        if np.isfinite(k["all"]).all():
            assert k["p"][2] > 0                                          # in front of the camera
            assert np.linalg.eigvalsh(k["S"]).min() >= -1e-12 * np.trace(k["S"])
        else:
            assert np.isnan(k["all"]).all()                               # the anchor clone has left the window
    assert list(per_pose) == [p for p in poses if p in per_pose]         # in pose order
    # the same loop through the Python mirror (as tests/test_gpu_vio_driver.py::test_cpp_dataset_driver_on_an_asl_directory runs it)
    fe = larvio_amd.ImageProcessor(fcfg, gpu_ctx); assert fe.initialize()
    be = larvio_amd.LarVio(dict(bcfg, max_features=300), gpu_ctx); assert be.initialize()
    imu2 = imu_all.copy(); imu2["t"] = t_imu
    drv = VioDriver(fe, be, imu2)
    want = []
    for t, (_, img) in zip(t_img, frames):
        hi = int(np.count_nonzero(t_imu - float(t) < 0.05))
        has, upd = drv.step(float(t), hi, img=img)
        if upd:
            ids, anc, pos, cov = be.get_features_in_camera()
            assert np.array_equal(ids, be.features()[0])
            want.append(("%.9f" % be.state()["t"], ids, pos, cov))
    be.close(); fe.close()
    assert [w[0] for w in want] == poses
    n_lines = 0; most = 0
    for stamp, ids, pos, cov in want:
        got = per_pose.get(stamp, [])
        assert len(got) == len(ids) and [k["id"] for k in got] == ids.tolist()      # one line per in-state feature, in the getter's order
        for k, p, S_ in zip(got, pos, cov):
            assert np.array_equal(k["p"], p, equal_nan=True) and np.array_equal(k["all"][3:], S_.ravel()[[0, 1, 2, 4, 5, 8]], equal_nan=True)
        n_lines += len(ids); most = max(most, len(ids))
    assert n_lines == len(lines) and most >= 3
    print("%d lines after %d of %d poses, up to %d features in the state" % (len(lines), len(per_pose), len(poses), most))
    r0 = subprocess.run(base + ["--tum", tum0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and open(tum0).read() == open(tum).read()      # the trajectory does not notice the getter
    out2 = str(tmp_path / "depth_pipelined.txt")
    r2 = subprocess.run(base + ["--depth-out", out2, "--pipelined"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert open(out2).read() == open(out).read()                         # lvk_vio_pipe: the same lines from the odometry callback
    out3 = str(tmp_path / "depth_adapter.txt")
    r3 = subprocess.run([os.path.join(ROOT, "adapter", "adapter_main")] + args + ["--depth-out", out3], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 0, r3.stdout + r3.stderr
    assert [l.split()[1:] for l in open(out3).read().splitlines()] == [l.split()[1:] for l in lines]      # the adapter's getter: the same numbers
