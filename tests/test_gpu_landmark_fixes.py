"""lvk_ekf_add_landmark_obs and what goes with it on simulated messages (tests/feature_sim.py, sw_size 10, the messages of the fix
tests): a filter that is never handed a batch keeps its bits, so does one that is handed empty batches only; blocking and deferred runs
give the same bytes and reports; the queue's rules (STALE, NO_CLONE, the waiting batch, capacity, the shard refusal, an add while an
update is unwaited); one applied batch gives the restatement's covariance and state (tests/landmark_fix_ref.py) inside the derived
bound times a margin; eight true landmarks per message keep the position error bounded and consistent and shrink the position block;
with 30 % grossly wrong associations the 99.9 % gate rejects exactly what the restatement rejects.

Where the restatement's inputs come from: as in tests/test_gpu_fixes.py, the third message of the run runs no measurement update and no
pruning (asserted), so a twin that processes the same three messages without the batch ends, bit for bit, in the covariance, clones and
extrinsics the batch meets."""
import ctypes as C
import numpy as np
import pytest

from tests import landmark_fix_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
SIGMA = 1e-3                   # normalised image noise of the simulated landmark observations
CHI2_3_999 = 16.27             # the 99.9 % quantile of chi-square with 3 degrees of freedom
# filter level against the restatement: the margin on the stage bound.  The host's state injection has its own allowance below (one
# rounding per sum, a few per quaternion product), so the stage bound itself is asked for; measured on an MI355X: 0.28 on P, 0.001 on
# the state (PARITY.md)
MARGIN = 1.0


def _snap(gpu):
    s = gpu.state(); c = gpu.counters()
    return dict(state=np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]]), P=gpu.cov(),
                counters=np.array([c[k] for k in sorted(c)]), cd=c, clones=gpu.clones(), p=s["p"], t=s["t"])


def _drive(ctx, sim, before=None, after=None, deferred=False, n_msgs=None, setup=None, touch=False):
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
        if before or after or touch:
            reports.append(gpu.take_landmark_reports())
        if after:
            after(gpu, k, snaps[-1])
    stats = gpu.landmark_stats() if (before or after or touch) else None
    gpu.close()
    return snaps, reports, stats


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x["state"].view(np.uint64), y["state"].view(np.uint64))
        assert x["P"].shape == y["P"].shape and np.array_equal(x["P"].view(np.uint64), y["P"].view(np.uint64))
        assert np.array_equal(x["counters"], y["counters"]) and x["clones"].tobytes() == y["clones"].tobytes()


def _true_landmarks(sim, rng, t, k, wrong=0):
    """k points 3 - 8 m in front of the TRUE camera at time t, their true projections plus N(0, SIGMA^2); the first `wrong` observations
    belong to other points (moved 0.2 - 0.4 in the image: gross mismatches) -> (p_w, uv)"""
    tr = sim["traj"]
    Rwb, pwb = tr.R_wb(t), tr.p_wb(t)
    z = rng.uniform(3.0, 8.0, k); uv = rng.uniform(-0.4, 0.4, (k, 2))
    pc = np.column_stack([uv[:, 0] * z, uv[:, 1] * z, z])
    pw = pwb + (Rwb @ (tr.R_cb.T @ (pc - tr.t_cb).T)).T
    uv = uv + rng.normal(0, SIGMA, (k, 2))
    uv[:wrong] += rng.choice([-1, 1], (wrong, 2)) * rng.uniform(0.2, 0.4, (wrong, 2))
    return pw, uv


@pytest.fixture(scope="module")
def sim():
    from tests import feature_sim as S
    return S.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)


@pytest.fixture(scope="module")
def plain(gpu_ctx, sim):
    """a run that never calls the new functions"""
    return _drive(gpu_ctx, sim)[0]


def test_no_batch_and_only_empty_batches_leave_the_bits_of_a_run_without_the_new_functions(gpu_ctx, sim, plain):
    assert len(plain) >= 40 and plain[-1]["counters"].sum() > 0
    snaps, reports, stats = _drive(gpu_ctx, sim, touch=True, setup=lambda gpu: gpu.set_landmark_options(R.GATE_999, 0.2))
    _same(snaps, plain)
    assert sum(len(r) for r in reports) == 0 and set(stats.values()) == {0}

    def after(gpu, k, s):
        gpu.add_landmark_obs(np.zeros((0, 3)), np.zeros((0, 2)), SIGMA, clone_id=int(s["clones"][-1]["id"]), tag=k)
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after)
    _same(snaps, plain)
    rep = np.concatenate(reports)
    assert len(rep) == len(plain) - 1 and np.all(rep["status"] == 1) and np.all(rep["n_obs"] == 0) and list(rep["tag"]) == list(range(len(plain) - 1))
    assert stats["queued"] == len(plain) and stats["all_rejected"] == len(plain) - 1 and stats["waiting"] == 1 and stats["used"] == 0


def test_one_applied_batch_gives_the_restatements_covariance_and_state(gpu_ctx, sim, plain):
    from tests.landmark_cov_ref import quat_mul, small_angle_quat, quat_to_rot
    assert all(plain[2]["cd"][k] == plain[1]["cd"][k] for k in ("hybrid", "msckf", "zupt"))
    assert len(plain[2]["clones"]) == 3 and plain[2]["P"].shape == (40, 40)
    A = plain[2]
    target = A["clones"][1]
    rng = np.random.default_rng(20261021)
    pw, uv = _true_landmarks(sim, rng, float(target["time"]), 9, wrong=2)
    cov = np.array([[4e-4, 1e-4, 0], [1e-4, 9e-4, -2e-4], [0, -2e-4, 2.5e-4]])

    def before(gpu, k):
        if k == 2:
            gpu.add_landmark_obs(pw, uv, SIGMA, cov_w=cov, clone_id=int(target["id"]), tag=11)
    snaps, reports, stats = _drive(gpu_ctx, sim, before=before, n_msgs=3, setup=lambda gpu: gpu.set_landmark_options(R.GATE_999, 0.1))
    _same(snaps[:2], plain[:2])
    B = snaps[2]; rep = reports[2]
    job = R.make_job(22 + 6, target["q"], target["p"], A["state"][17:26], A["state"][26:29], gate=R.GATE_999 * R.CHI2_005_2, min_depth=0.1)
    obs = np.zeros(9, R.OBS_DTYPE); obs["p_w"] = pw; obs["uv"] = uv; obs["sigma"] = SIGMA; obs["cov_w"] = cov.ravel()
    t = R.batch_tracked(A["P"], job, obs)
    live = t["status"] != R.BEHIND
    assert np.all(np.abs(t["gamma"][live].astype(np.float64) - job["gate"]) > 1e-6 * job["gate"])
    assert len(rep) == 1 and rep[0]["status"] == 0 and rep[0]["tag"] == 11 and rep[0]["clone_id"] == target["id"] and stats["applied"] == 1
    assert (rep[0]["n_obs"], rep[0]["n_used"], rep[0]["n_gated"], rep[0]["n_behind"]) == (9, t["n_used"], t["n_gated"], t["n_behind"]) and t["n_gated"] >= 1
    assert abs(LD(rep[0]["gamma"]) - t["gamma_b"]) <= MARGIN * t["e_gamma_b"]
    assert all(B["cd"][k] == A["cd"][k] for k in ("hybrid", "msckf", "zupt"))                # nothing but the batch separates B from A
    wP = R.worst_ratio(B["P"].astype(LD) - t["P"], t["e_P"])
    assert np.array_equal(B["P"].view(np.uint64), np.ascontiguousarray(B["P"].T).view(np.uint64))
    dx, e = t["dx"], t["e_dx"]
    u = R.U
    w = 0.0
    for lo_s, lo_x in ((5, 3), (8, 6), (11, 9), (14, 12), (26, 18)):          # v p bg ba of the IMU state and t_c_b: additive, one rounding of the sum on top
        ref = A["state"][lo_s:lo_s + 3].astype(LD) + dx[lo_x:lo_x + 3]
        w = max(w, R.worst_ratio(B["state"][lo_s:lo_s + 3] - ref, e[lo_x:lo_x + 3] + u * np.abs(ref)))
    for c in range(3):
        ref = A["clones"][c]["p"].astype(LD) + dx[25 + 6 * c:28 + 6 * c]
        w = max(w, R.worst_ratio(B["clones"][c]["p"] - ref, e[25 + 6 * c:28 + 6 * c] + u * np.abs(ref)))
    for qa, qb, col in [(A["state"][1:5], B["state"][1:5], 0)] + [(A["clones"][c]["q"], B["clones"][c]["q"], 22 + 6 * c) for c in range(3)]:
        ref = quat_mul(small_angle_quat(dx[col:col + 3]), qa.astype(LD))
        w = max(w, R.worst_ratio(qb - ref, np.max(e[col:col + 3]) + 8 * u))
    Re = A["state"][17:26].reshape(3, 3).astype(LD) @ quat_to_rot(small_angle_quat(dx[15:18])).T      # R_b2c <- R_b2c R(d_theta_e)^T
    w = max(w, R.worst_ratio(B["state"][17:26].reshape(3, 3) - Re, 2 * np.max(e[15:18]) + 16 * u))
    print("one applied batch: worst |error| / bound P %.3f, state %.3f; used %d gated %d; gamma %.4f" % (wP, w, t["n_used"], t["n_gated"], rep[0]["gamma"]))
    assert np.max(np.abs(dx[28:34])) > 1e-6                               # the batch moved its clone
    assert wP <= MARGIN and w <= MARGIN


def _landmarks_every_message(ctx, sim, deferred, wrong=0, k_pts=8):
    rng = np.random.default_rng(20261022)
    expected = {}

    def after(gpu, k, s):
        c = s["clones"][-1]
        pw, uv = _true_landmarks(sim, rng, float(c["time"]), k_pts, wrong=wrong)
        gpu.add_landmark_obs(pw, uv, SIGMA, clone_id=int(c["id"]), tag=k)
        expected[k] = (pw, uv)
    out = _drive(ctx, sim, after=after, deferred=deferred, setup=lambda gpu: gpu.set_landmark_options(R.GATE_999, 0.1))
    return out + (expected,)


@pytest.fixture(scope="module")
def mapped_run(gpu_ctx, sim):
    return _landmarks_every_message(gpu_ctx, sim, False)


def _d2(snaps, sim):
    out = []
    for s in snaps:
        e = s["p"] - sim["traj"].p_wb(s["t"])
        out.append((float(e @ np.linalg.solve(s["P"][6:9, 6:9], e)), float(np.linalg.norm(e))))
    return np.array(out)


def test_true_landmarks_bound_the_position_error_and_shrink_the_position_block(sim, plain, mapped_run):
    snaps, reports, stats, _ = mapped_run
    rep = np.concatenate(reports)
    assert len(rep) == len(snaps) - 1 and np.all(rep["status"] == 0) and np.all(rep["n_obs"] == 8), rep
    assert stats["applied"] == len(rep) and stats["waiting"] == 1 and stats["used"] + stats["gated"] + stats["behind"] == stats["obs"] == 8 * len(rep)
    d = _d2(snaps[5:], sim); dp = _d2(plain[5:], sim)
    tr = lambda s: float(np.trace(s["P"][6:9, 6:9]))
    print("with landmarks: median d2 %.2f, largest |error| %.4f m, final trace %.3g, used %d gated %d; without: median d2 %.2f, largest |error| %.4f m, final trace %.3g" %
          (np.median(d[:, 0]), d[:, 1].max(), tr(snaps[-1]), stats["used"], stats["gated"], np.median(dp[:, 0]), dp[:, 1].max(), tr(plain[-1])))
    assert np.median(d[:, 0]) < CHI2_3_999
    assert d[:, 1].max() < 0.05                       # 8 points at 3 - 8 m seen to 1e-3: a few millimetres; the start is known to centimetres
    assert tr(snaps[-1]) < tr(plain[-1])


def test_blocking_and_deferred_runs_give_the_same_bytes(gpu_ctx, sim, mapped_run):
    snaps, reports, stats, _ = _landmarks_every_message(gpu_ctx, sim, True)
    _same(snaps, mapped_run[0])
    assert np.concatenate(reports).tobytes() == np.concatenate(mapped_run[1]).tobytes() and stats == mapped_run[2]


def test_wrong_associations_are_gated_as_the_restatement_gates_them(gpu_ctx, sim):
    """30 % of every batch of 10 belongs to other points; the filter level comparison of n_gated runs on the first batch, whose inputs a
    twin run supplies (the later ones meet a state that already differs from any twin's)"""
    snaps, reports, stats, expected = _landmarks_every_message(gpu_ctx, sim, False, wrong=3, k_pts=10)
    rep = np.concatenate(reports)
    d = _d2(snaps[5:], sim)
    print("30 %% wrong: median d2 %.2f, largest |error| %.4f m, gated %d of %d" % (np.median(d[:, 0]), d[:, 1].max(), stats["gated"], stats["obs"]))
    assert np.median(d[:, 0]) < CHI2_3_999
    assert np.all(rep["n_gated"] >= 3) and stats["gated"] <= 3 * len(rep) + len(rep) // 4          # the wrong ones go, and hardly anything else
    # the batch queued after message 0 is applied in message 1, which (asserted) runs no update of its own before it
    A = snaps[0]
    twin = _drive(gpu_ctx, sim, n_msgs=2)[0]
    assert all(twin[1]["cd"][k] == twin[0]["cd"][k] for k in ("hybrid", "msckf", "zupt")) and len(twin[1]["clones"]) == 2
    T = twin[1]; target = T["clones"][0]
    assert target["id"] == A["clones"][-1]["id"]
    pw, uv = expected[0]
    job = R.make_job(22, target["q"], target["p"], T["state"][17:26], T["state"][26:29], gate=R.GATE_999 * R.CHI2_005_2, min_depth=0.1)
    obs = np.zeros(10, R.OBS_DTYPE); obs["p_w"] = pw; obs["uv"] = uv; obs["sigma"] = SIGMA
    t = R.batch_tracked(T["P"], job, obs)
    assert np.all(np.abs(t["gamma"].astype(np.float64) - job["gate"]) > 1e-6 * job["gate"])
    assert rep[0]["tag"] == 0 and (rep[0]["n_used"], rep[0]["n_gated"], rep[0]["n_behind"]) == (t["n_used"], t["n_gated"], t["n_behind"]) and t["n_gated"] == 3


def test_queue_rules_and_refusals(gpu_ctx, sim, plain):
    import larvio_amd
    from larvio_amd._lib import LvkError
    times = [s["clones"][-1]["time"] for s in plain]
    one = (np.array([[0.0, 0, 5]]), np.array([[0.0, 0]]), SIGMA)
    seen = {}

    def after(gpu, k, s):
        cl = s["clones"]
        if k == 19:
            gone = sorted(set(range(int(cl[-1]["id"]))) - set(cl["id"].tolist()))[0]
            gpu.add_landmark_obs(*one, clone_id=gone, tag=1)                                               # an id pruned earlier: STALE
            gpu.add_landmark_obs(*one, time=float(cl[0]["time"]) - 1.0, tag=2)                             # older than the oldest clone: STALE
            gpu.add_landmark_obs(*one, time=0.5 * (float(cl[-2]["time"]) + float(cl[-1]["time"])), tag=3)  # strictly between two clones: NO_CLONE
            gpu.add_landmark_obs(*one, time=float(times[21]), tag=4)                                       # the clone of message 21: waits
        if k == 20:
            seen["waiting"] = gpu.landmark_stats()["waiting"]
    snaps, reports, stats = _drive(gpu_ctx, sim, after=after, n_msgs=23)
    by_tag = {int(r["tag"]): (k, r) for k, rs in enumerate(reports) for r in rs}
    assert sorted(by_tag) == [1, 2, 3, 4]
    assert by_tag[1][1]["status"] == 3 and by_tag[2][1]["status"] == 3 and by_tag[1][0] == by_tag[2][0] == 20 and by_tag[1][1]["clone_id"] == -1
    assert by_tag[3][1]["status"] == 4 and by_tag[3][0] == 20
    assert seen["waiting"] == 1 and by_tag[4][0] == 21 and by_tag[4][1]["status"] in (0, 1) and by_tag[4][1]["clone_id"] == snaps[21]["clones"][-1]["id"]
    assert stats["queued"] == 4 and stats["stale"] == 2 and stats["no_clone"] == 1 and stats["waiting"] == 0

    gpu = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert gpu.initialize()
    gpu.set_state(*sim["init"])

    def refused(status, *a, **kw):
        args = a if a else one
        with pytest.raises(LvkError) as ei:
            gpu.add_landmark_obs(*args, **kw)
        assert "status %d" % status in str(ei.value) and "lvk_ekf_add_landmark_obs" in str(ei.value), str(ei.value)
    refused(1, np.array([[0.0, np.nan, 5]]), one[1], SIGMA)
    refused(1, one[0], np.array([[np.inf, 0.0]]), SIGMA)
    refused(1, one[0], one[1], 0.0)
    refused(1, one[0], one[1], SIGMA, cov_w=np.array([[1.0, 2, 0], [2, 1, 0], [0, 0, 1]]))
    refused(1, time=np.inf)
    refused(1, clone_id=-2)
    refused(3, np.zeros((1025, 3)) + [0, 0, 5], np.zeros((1025, 2)), SIGMA)                # more than 1024 observations
    for bad in ((np.nan, 0.1), (1.0, -0.1), (1.0, np.nan)):
        with pytest.raises(LvkError):
            gpu.set_landmark_options(*bad)
    assert gpu.landmark_stats()["queued"] == 0
    imu = sim["imu"]; lo = 0
    for k, (ts, m) in enumerate(sim["msgs"][:3]):                                          # a deferred update is pending: refused until something has waited for it
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = gpu.processFeaturesAsync((ts, m), b); lo += len(b) - len(rest)
        if k == 2:
            refused(1)
            gpu.wait()
            gpu.add_landmark_obs(*one, time=1e9)
        else:
            gpu.wait()
    for k in range(15):
        gpu.add_landmark_obs(*one, time=1e9)
    assert gpu.landmark_stats()["waiting"] == 16
    refused(3, time=1e9)                                                                   # the 17th batch
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 0)      # never called here
    fn = C.cast(cb, C.c_void_p)
    with pytest.raises(LvkError) as ei:
        gpu.set_shard(0, 1, fn, None, keepalive=cb)                                        # a transport is refused while batches wait ...
    assert "status 4" in str(ei.value)
    gpu.close()
    gpu = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert gpu.initialize()
    gpu.set_shard(0, 1, fn, None, keepalive=cb)
    refused(4)                                                                             # ... and a batch while a transport is set
    gpu.close()
