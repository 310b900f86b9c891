"""The JSON line `bench.py --full` prints, as committed under profiles/ from the last MI355X run: every field of the driver's contract
is there with the right type (bench.py itself needs a GPU; this keeps the contract from drifting unnoticed)."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_bench_line_has_the_contract_fields():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_bench.json")))
    assert files
    d = json.loads(open(files[-1]).read().strip().splitlines()[-1])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int), ("ms_per_step", float),
                 ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict), ("roofline", dict),
                 ("cpu_baseline", dict)):
        assert k in d and isinstance(d[k], t), k
    assert "vs_baseline" in d and d["vs_baseline"] is None          # BASELINE.md publishes no number for this metric
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic" and d["n_gpus"] == 1
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5 and (r["traffic"] is None or r["traffic"] > 0)
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == d["unit"] and c["sample"]
    assert abs(d["value"] - d["steps"] / (d["ms_per_step"] * 1e-3 * d["steps"]) * d["n_gpus"]) < 0.01 * d["value"]
    # round 3: the metric is quoted at ~150 live tracks; the adapter-reachable schedule, the TSQR roofline and the configs[4]-depth probe ride along
    assert d["config"]["live_tracks"] >= 145
    a = d["adapter_path"]
    assert a["unit"] == d["unit"] and 0 < a["value"] < d["value"] and a["pose_read_one_frame_late"]["value"] >= 0.9 * a["value"]
    q = d["roofline_qr"]
    assert q["kernel"].startswith("k_qr_sparse") and q["flops_per_launch"] > 0 and abs(q["frac"] - q["achieved"] / q["peak"]) < 1e-5
    # round 3, final state: the pipelined driver's early erase counts were all confirmed; the timed region holds whole publish cycles
    ec = d["erase_counts_taken_early"]
    assert ec["since_start"] > 0 and ec["found_wrong"] == 0
    assert d["config"]["timed_region_alignment"].startswith("starts on a publish frame")
    pr = d["sharded_update_probe"]
    assert pr["cpu_baseline"]["kind"] == "port" and pr["cpu_baseline"]["value"] > 0 and pr["rccl_loopback"]["shard"]["exchanges"] == pr["rccl_loopback"]["shard"]["sharded_updates"] > 0


def test_bench_source_keeps_the_timed_region_bracketed():
    src = open(os.path.join(ROOT, "bench.py")).read()
    i0 = src.index("t_begin = time.perf_counter()"); i1 = src.index("elapsed = time.perf_counter() - t_begin")
    before, timed = src[:i0], src[i0:i1]
    assert "dist.barrier()" in before[-400:] and "torch.cuda.synchronize()" in before[-400:]
    assert "torch.cuda.synchronize()" in timed and "dist.barrier()" in timed and "run.drain()" in timed      # every queued update completes inside
    assert "oracle" not in timed                                   # the CPU baseline is timed outside


def test_bench_source_reaches_the_stated_steady_state_before_timing():
    """The timed region must not depend on --warmup to fill the window (round-1 finding): the pre-roll is a separate, untimed phase
    that refuses to hand over until the window has cycled and the H P GEMM was bracketed over >= 20 updates; the image is handed
    over as a host buffer in the headline pass."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    main = src[src.index("def main()"):]
    assert main.index("preroll(run, frames, None") < main.index("timed(run, frames, None")
    pre = src[src.index("def preroll("):src.index("def timed(")]
    assert "sw_size - 2" in pre and 'c["msckf"] >= 2' in pre and "raise SystemExit" in pre and "no value printed" in pre
    assert "preroll(run, frames, None, n_pre_max, sw, 20, warmup=W, period=period)" in main
    assert "n_cpu = 0 if" in main and "else 300" in main                       # >= 200 steady-state CPU frames at the metric's configuration


def test_every_committed_counter_table_parses():
    """bench.py reads roofline.traffic from the newest profiles/r*_{a,c5}_pmc_fetch_size.csv; kernel names in those tables carry commas
    (k_fe_lk_both<21, 1>): a naive split broke `--config 5` once (round 6)"""
    import glob
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_fetch_size.csv")))
    assert files
    got = {os.path.basename(f): bench.pmc_lk_traffic(f) for f in files}
    assert got["r6_n_c5_pmc_fetch_size.csv"] > 4e7 and got["r6_i_a_pmc_fetch_size.csv"] > 4e6


def test_bench_options_for_a_plain_run_and_its_outputs():
    """--full gates everything measured beside the headline; --dump-outputs writes float32 / float64 arrays, a seeded sample of any that
    would take the dump past its cap (same indices on every run)"""
    import subprocess
    import sys
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec); spec.loader.exec_module(bench)
    main = open(os.path.join(ROOT, "bench.py")).read()
    main = main[main.index("def main()"):]
    for gate in ("cpp_leg = args.full and", "if args.full and not args.no_device_pass", "if args.full and not args.sequential and not args.no_adapter_pass",
                 "if args.full and not args.unaligned", "if args.full and not args.no_shard_probe", "n_cpu = 0 if (not args.full"):
        assert gate in main, gate
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        big = np.arange(bench.DUMP_MAX_BYTES // 8 + 1000, dtype=np.float64)
        bench.dump_outputs(d, dict(a=np.ones((3, 4), np.float32), b=np.arange(5.0), big=big))
        assert np.load(os.path.join(d, "a.npy")).dtype == np.float32 and np.array_equal(np.load(os.path.join(d, "b.npy")), np.arange(5.0))
        s, idx = np.load(os.path.join(d, "big.npy")), np.load(os.path.join(d, "big_index.npy"))
        assert 0 < s.size < big.size and np.array_equal(s, big[idx.astype(np.int64)])
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 * 10 ** 6
        with tempfile.TemporaryDirectory() as d2:
            bench.dump_outputs(d2, dict(a=np.ones((3, 4), np.float32), b=np.arange(5.0), big=big))
            assert np.array_equal(np.load(os.path.join(d2, "big_index.npy")), idx)
