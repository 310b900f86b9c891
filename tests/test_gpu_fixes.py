"""lvk_ekf_add_fix and what goes with it on simulated messages (tests/feature_sim.py, sw_size 10, the messages of the keyframe tests): a
filter that is never handed a fix keeps its bits, so does one whose only fix is gated out; one applied fix gives the restatement's
covariance and state (tests/fix_ref.py) inside the derived bound; position fixes from the true trajectory shrink the position block and
keep the estimate consistent; every status is reported as such; blocking and deferred runs give the same bytes; the refusals.

Where the restatement's inputs come from: fixes are applied inside an update, behind the message's propagation and augmentation.  The
third message of the run runs no measurement update and no pruning (asserted: the counters stand), so a twin that processes the same
three messages without the fix ends, bit for bit, in the covariance and clones the fix meets: its lvk_ekf_get_cov / lvk_ekf_get_clones
are read "just before" in that sense."""
import ctypes as C
import numpy as np
import pytest

from tests import fix_ref as F

pytestmark = pytest.mark.gpu
LD = F.LD
SIGMA_FIX = 0.05               # m: the standard deviation of the simulated position fixes (a good RTK / motion-capture fix); belongs to this test
GATE_999 = 16.27 / F.CHI2_005[3]      # gate_scale that makes the 3-row gate the 99.9 % quantile the sibling tests use


def _snap(gpu):
    s = gpu.state(); c = gpu.counters()
    return dict(state=np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]]), P=gpu.cov(),
                counters=np.array([c[k] for k in sorted(c)]), cd=c, clones=gpu.clones(), p=s["p"], t=s["t"])


def _drive(ctx, sim, before=None, after=None, deferred=False, n_msgs=None, setup=None):
    """before(gpu, k) / after(gpu, k, snap): called around message k; -> (snapshots after every message, all reports, final stats)"""
    import larvio_amd
    gpu = larvio_amd.LarVio(sim["cfg"], ctx); assert gpu.initialize()
    if setup:
        setup(gpu)
    gpu.set_state(*sim["init"])
    imu = sim["imu"]; lo = 0; snaps = []; reports = []
    for k, (ts, m) in enumerate(sim["msgs"][:n_msgs]):
        if before:
            before(gpu, k)
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = (gpu.processFeaturesAsync if deferred else gpu.processFeatures)((ts, m), b)
        lo += len(b) - len(rest)
        snaps.append(_snap(gpu))
        if before or after:
            reports.append(gpu.take_fix_reports())
        if after:
            after(gpu, k, snaps[-1])
    stats = gpu.fix_stats() if (before or after) else None
    gpu.close()
    return snaps, reports, stats


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["state"].view(np.uint64), y["state"].view(np.uint64))
        assert x["P"].shape == y["P"].shape and np.array_equal(x["P"].view(np.uint64), y["P"].view(np.uint64))
        assert np.array_equal(x["counters"], y["counters"]) and x["clones"].tobytes() == y["clones"].tobytes()


@pytest.fixture(scope="module")
def sim():
    from tests import feature_sim as S
    return S.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)


@pytest.fixture(scope="module")
def plain(gpu_ctx, sim):
    """a run that never calls the new functions"""
    return _drive(gpu_ctx, sim)[0]


def test_no_fix_ever_queued_leaves_the_bits_of_a_run_without_the_new_functions(gpu_ctx, sim, plain):
    assert len(plain) >= 40 and plain[-1]["counters"].sum() > 0
    snaps, reports, stats = _drive(gpu_ctx, sim, before=lambda gpu, k: gpu.fix_stats(), setup=lambda gpu: gpu.set_fix_options(GATE_999, 0.2))
    _same(snaps, plain)
    assert sum(len(r) for r in reports) == 0 and set(stats.values()) == {0}


def test_a_fix_100_m_off_is_gated_and_the_filter_keeps_the_twins_bits(gpu_ctx, sim, plain):
    def after(gpu, k, s):
        if k == 19:
            c = s["clones"][-1]
            gpu.add_fix(c["p"] + np.array([100.0, 0, 0]), SIGMA_FIX ** 2 * np.eye(3), clone_id=int(c["id"]), tag=7)
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after, setup=lambda gpu: gpu.set_fix_options(GATE_999, 0.0))
    rep = np.concatenate(reports)
    assert len(rep) == 1 and len(reports[20]) == 1 and rep[0]["tag"] == 7 and rep[0]["status"] == 1 and rep[0]["gamma"] > 16.27
    assert rep[0]["clone_i"] == plain[19]["clones"][-1]["id"] and rep[0]["clone_j"] == -1
    assert stats["queued"] == 1 and stats["gated"] == 1 and stats["applied"] == 0 and stats["waiting"] == 0
    _same(snaps, plain)


def test_one_applied_fix_gives_the_restatements_covariance_and_state(gpu_ctx, sim, plain):
    from tests.landmark_cov_ref import quat_mul, small_angle_quat, quat_to_rot
    # the twin: message 2 runs no update and no pruning, so its end state is what the fix meets
    assert all(plain[2]["cd"][k] == plain[1]["cd"][k] for k in ("hybrid", "msckf", "zupt"))
    assert len(plain[2]["clones"]) == 3 and plain[2]["P"].shape == (40, 40)
    A = plain[2]
    target = A["clones"][1]
    lever = np.array([0.10, -0.05, 0.20])
    Rm = np.array([[2.5e-3, 5e-4, 0], [5e-4, 3.0e-3, -4e-4], [0, -4e-4, 2.0e-3]])
    z = (target["p"].astype(LD) + quat_to_rot(target["q"].astype(LD)) @ lever + np.array([0.01, -0.005, 0.0075], LD)).astype(np.float64)

    def before(gpu, k):
        if k == 2:
            gpu.add_fix(z, Rm, clone_id=int(target["id"]), lever=lever, tag=11)
    snaps, reports, stats = _drive(gpu_ctx, sim, before=before, n_msgs=3)
    _same(snaps[:2], plain[:2])
    B = snaps[2]; rep = reports[2]
    assert len(rep) == 1 and rep[0]["status"] == 0 and rep[0]["tag"] == 11 and rep[0]["clone_i"] == target["id"] and stats["applied"] == 1
    cols, H, r = F.fix_rows(F.POSITION, [F.clone_pose(target, 1)], 0.0, lever, z)
    t = F.update_tracked(A["P"], cols, H, r, Rm, F.CHI2_005[3])
    assert t["status"] == 0
    assert abs(LD(rep[0]["gamma"]) - t["gamma"]) <= t["e_gamma"]
    assert all(B["cd"][k] == A["cd"][k] for k in ("hybrid", "msckf", "zupt"))                # ... with the fix as well: nothing but the fix separates B from A
    wP = F.worst_ratio(B["P"].astype(LD) - t["P"], t["e_P"])
    assert np.array_equal(B["P"].view(np.uint64), np.ascontiguousarray(B["P"].T).view(np.uint64))
    dx, e = t["dx"], t["e_dx"]
    u = F.U
    w = 0.0
    # additive parts: v (3..5), p (6..8), bg, ba of the IMU state (state vector: t q v p bg ba ...), p of every clone; one rounding of the sum on top
    for lo_s, lo_x in ((5, 3), (8, 6), (11, 9), (14, 12)):
        ref = A["state"][lo_s:lo_s + 3].astype(LD) + dx[lo_x:lo_x + 3]
        w = max(w, F.worst_ratio(B["state"][lo_s:lo_s + 3] - ref, e[lo_x:lo_x + 3] + u * np.abs(ref)))
    poses = [(A["state"][1:5], B["state"][1:5], 0)] + [(A["clones"][c]["q"], B["clones"][c]["q"], 22 + 6 * c) for c in range(3)]
    for c in range(3):
        ref = A["clones"][c]["p"].astype(LD) + dx[25 + 6 * c:28 + 6 * c]
        w = max(w, F.worst_ratio(B["clones"][c]["p"] - ref, e[25 + 6 * c:28 + 6 * c] + u * np.abs(ref)))
    # attitudes, through the injection: q <- small_angle_quat(d_theta) * q; the product's own rounding is a few u on numbers <= 1
    for qa, qb, col in poses:
        ref = quat_mul(small_angle_quat(dx[col:col + 3]), qa.astype(LD))
        w = max(w, F.worst_ratio(qb - ref, np.max(e[col:col + 3]) + 8 * u))
    print("one applied fix: worst |error| / bound P %.3f, state %.3f; gamma %.4f" % (wP, w, rep[0]["gamma"]))
    assert np.max(np.abs(dx[25 + 6:28 + 6])) > 1e-5                       # the fix moved its clone
    assert wP <= 1.0 and w <= 1.0


@pytest.fixture(scope="module")
def fixed_run(gpu_ctx, sim):
    return _fix_every_fifth(gpu_ctx, sim, False)


def _fix_every_fifth(ctx, sim, deferred):
    """a position fix on the newest clone after every fifth message, from the true trajectory plus N(0, SIGMA_FIX^2 I); it is applied by the
    next message"""
    rng = np.random.default_rng(20261020)

    def after(gpu, k, s):
        if k % 5 == 0 and k > 0:
            c = s["clones"][-1]
            gpu.add_fix(sim["traj"].p_wb(c["time"]) + rng.normal(0, SIGMA_FIX, 3), SIGMA_FIX ** 2 * np.eye(3), clone_id=int(c["id"]), tag=k)
    return _drive(ctx, sim, after=after, deferred=deferred, setup=lambda gpu: gpu.set_fix_options(GATE_999, 0.0))


def test_position_fixes_shrink_the_position_block_and_stay_consistent(sim, plain, fixed_run):
    snaps, reports, stats = fixed_run
    rep = np.concatenate(reports)
    assert len(rep) == 7 and np.all(rep["status"] == 0) and list(rep["tag"]) == [5, 10, 15, 20, 25, 30, 35], rep
    assert stats["queued"] == 7 and stats["applied"] == 7 and stats["waiting"] == 0
    tr = lambda s: float(np.trace(s["P"][6:9, 6:9]))
    for k in range(6, len(snaps)):
        assert tr(snaps[k]) < tr(plain[k]), (k, tr(snaps[k]), tr(plain[k]))
    last = snaps[-1]
    e = last["p"] - sim["traj"].p_wb(last["t"])
    d2 = float(e @ np.linalg.solve(last["P"][6:9, 6:9], e))
    print("final position: error %s m, sigma %s m, d2 %.2f (plain run: trace %.3g against %.3g with fixes)" %
          (np.array2string(e, precision=4), np.array2string(np.sqrt(np.diag(last["P"][6:9, 6:9])), precision=4), d2, tr(plain[-1]), tr(last)))
    assert d2 < 16.27


def test_blocking_and_deferred_runs_give_the_same_bytes(gpu_ctx, sim, fixed_run):
    snaps, reports, stats = _fix_every_fifth(gpu_ctx, sim, True)
    _same(snaps, fixed_run[0])
    assert np.concatenate(reports).tobytes() == np.concatenate(fixed_run[1]).tobytes() and stats == fixed_run[2]


def test_every_status_is_reported_as_such(gpu_ctx, sim, plain):
    times = [s["clones"][-1]["time"] for s in plain]                      # the time of every message's own clone: IMU time stamps, the same in every run
    cov = SIGMA_FIX ** 2 * np.eye(3)
    truth = lambda t: sim["traj"].p_wb(t)
    seen = {}

    def after(gpu, k, s):
        cl = s["clones"]
        if k == 19:
            gone = sorted(set(range(int(cl[-1]["id"]))) - set(cl["id"].tolist()))[0]
            gpu.add_fix(truth(times[0]), cov, clone_id=gone, tag=1)                                     # an id pruned earlier: STALE
            gpu.add_fix(truth(times[0]), cov, time=float(cl[0]["time"]) - 1.0, tag=2)                   # older than the oldest clone: STALE
            tm = 0.5 * (float(cl[-2]["time"]) + float(cl[-1]["time"]))
            gpu.add_fix(truth(tm), cov, time=tm, tag=3)                                                 # between two clones, max_gap_s 0: NO_CLONE
            gpu.add_fix(truth(times[21]), cov, time=float(times[21]), tag=4)                            # the clone of message 21: waits, then applied
        if k == 20:
            seen["waiting"] = gpu.fix_stats()["waiting"]
        if k == 24:
            gpu.set_fix_options(GATE_999, 0.15)
            tm = 0.5 * (float(cl[-2]["time"]) + float(cl[-1]["time"]))
            seen["ij"] = (int(cl[-2]["id"]), int(cl[-1]["id"]))
            gpu.add_fix(truth(tm), cov, time=tm, tag=5)                                                 # the same, with a gap allowed: interpolated
            gpu.add_fix(truth(tm), 1e-2 * np.eye(6), time=tm, q=np.array([0.0, 0, 0, 1]), tag=6)        # a POSE fix is never interpolated: NO_CLONE
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after, setup=lambda gpu: gpu.set_fix_options(GATE_999, 0.0), n_msgs=27)
    by_tag = {int(r["tag"]): (k, r) for k, rs in enumerate(reports) for r in rs}
    assert sorted(by_tag) == [1, 2, 3, 4, 5, 6]
    assert by_tag[1][1]["status"] == 3 and by_tag[2][1]["status"] == 3 and by_tag[1][0] == by_tag[2][0] == 20
    assert by_tag[3][1]["status"] == 4 and by_tag[3][1]["clone_i"] == -1 and by_tag[3][0] == 20
    assert seen["waiting"] == 1 and by_tag[4][0] == 21 and by_tag[4][1]["status"] == 0 and by_tag[4][1]["clone_i"] == snaps[21]["clones"][-1]["id"]
    assert snaps[21]["clones"][-1]["time"] == times[21]
    k5, r5 = by_tag[5]
    assert k5 == 25 and r5["status"] == 0 and (r5["clone_i"], r5["clone_j"]) == seen["ij"] and abs(r5["a"] - 0.5) < 1e-9
    assert by_tag[6][1]["status"] == 4 and by_tag[6][1]["kind"] == 1
    assert stats == dict(queued=6, applied=2, gated=0, not_pd=0, stale=2, no_clone=2, waiting=0, interpolated=1)


def test_refusals(gpu_ctx, sim):
    import larvio_amd
    from larvio_amd._lib import LvkError
    cov = SIGMA_FIX ** 2 * np.eye(3)
    gpu = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert gpu.initialize()
    gpu.set_state(*sim["init"])

    def refused(status, **kw):
        args = dict(p=np.zeros(3), cov=cov); args.update(kw)
        with pytest.raises(LvkError) as ei:
            gpu.add_fix(**args)
        assert "status %d" % status in str(ei.value) and "lvk_ekf_add_fix" in str(ei.value), str(ei.value)
    refused(1, p=np.array([0, np.nan, 0]))
    refused(1, time=np.inf)
    refused(1, lever=np.array([np.inf, 0, 0]))
    refused(1, cov=np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]]))                       # not positive definite
    refused(1, cov=np.array([[1.0, 0.1, 0], [0.2, 1, 0], [0, 0, 1]]))                   # not symmetric
    refused(1, cov=np.eye(6), q=np.array([0, 0, 0, 1.001]))                             # not a unit quaternion
    refused(1, cov=np.diag([1.0, 1, 1, 1, 1, -1]), q=np.array([0, 0, 0, 1.0]))
    refused(1, clone_id=-2)
    f = np.zeros(1, larvio_amd.larvio.FIX); f["kind"] = 2; f["cov"][0] = np.eye(6); f["q"][0, 3] = 1
    assert larvio_amd.larvio._L().lvk_ekf_add_fix(gpu._h, f.ctypes.data_as(C.c_void_p)) == 1     # a bad kind
    with pytest.raises(LvkError):
        gpu.set_fix_options(np.nan, 0.0)
    with pytest.raises(LvkError):
        gpu.set_fix_options(1.0, -1.0)
    assert gpu.fix_stats()["queued"] == 0
    # a deferred update is pending: refused until something has waited for it
    imu = sim["imu"]; lo = 0
    for k, (ts, m) in enumerate(sim["msgs"][:3]):
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = gpu.processFeaturesAsync((ts, m), b); lo += len(b) - len(rest)
        if k == 2:
            refused(1)
            gpu.wait()
            gpu.add_fix(np.zeros(3), cov, time=1e9)                                      # accepted now (it will wait: newer than every clone)
        else:
            gpu.wait()
    # the 65th fix
    for k in range(63):
        gpu.add_fix(np.zeros(3), cov, time=1e9)
    assert gpu.fix_stats()["waiting"] == 64
    refused(3, time=1e9)
    # a transport is refused while fixes wait ...
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 0)      # never called here
    fn = C.cast(cb, C.c_void_p)
    with pytest.raises(LvkError) as ei:
        gpu.set_shard(0, 1, fn, None, keepalive=cb)
    assert "status 4" in str(ei.value)
    gpu.close()
    # ... and a fix while a transport is set
    gpu = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert gpu.initialize()
    gpu.set_shard(0, 1, fn, None, keepalive=cb)
    refused(4)
    gpu.close()
