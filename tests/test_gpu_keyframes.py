"""lvk_ekf_set_keyframe_export / lvk_ekf_take_keyframes / lvk_ekf_get_window_cov on simulated messages (tests/feature_sim.py, sw_size 10,
41 messages): the export is a pure observer (state, covariance and counters keep their bits), blocking and deferred runs give the same
records, every clone that leaves the window is exported exactly once with a link to a clone that is still there, the records' relative
poses and covariances are what their own poses and the covariance of that instant say, and the relative poses sit on the simulation's
true trajectory as their covariance says."""
import numpy as np
import pytest

from tests import pose_rel_ref as R

pytestmark = pytest.mark.gpu


def _drive(ctx, sim, on, deferred=False, window=False):
    """-> (snapshots after every message, records per message, window covariances per message)"""
    import larvio_amd
    gpu = larvio_amd.LarVio(sim["cfg"], ctx); assert gpu.initialize()
    if on is not None:
        gpu.set_keyframe_export(on)
    gpu.set_state(*sim["init"])
    imu = sim["imu"]; lo = 0; snaps = []; recs = []; win = []
    for ts, m in sim["msgs"]:
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = (gpu.processFeaturesAsync if deferred else gpu.processFeatures)((ts, m), b)
        lo += len(b) - len(rest)
        s = gpu.state(); c = gpu.counters()
        snaps.append(dict(state=np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]]), P=gpu.cov(),
                          counters=np.array([c[k] for k in sorted(c)]), clones=gpu.clones()))
        recs.append(gpu.take_keyframes())
        if window:
            win.append(gpu.get_window_cov())
    assert len(gpu.take_keyframes()) == 0                                  # drained
    gpu.close()
    return snaps, recs, win


@pytest.fixture(scope="module")
def sim():
    from tests import feature_sim as F
    return F.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)


@pytest.fixture(scope="module")
def run_on(gpu_ctx, sim):
    return _drive(gpu_ctx, sim, True, window=True)


@pytest.fixture(scope="module")
def run_off(gpu_ctx, sim):
    return _drive(gpu_ctx, sim, None)


def test_switch_has_no_side_effect_on_the_filter(run_on, run_off):
    assert len(run_on[0]) == len(run_off[0]) >= 40
    for a, b in zip(run_on[0], run_off[0]):
        assert np.array_equal(a["state"].view(np.uint64), b["state"].view(np.uint64))
        assert a["P"].shape == b["P"].shape and np.array_equal(a["P"].view(np.uint64), b["P"].view(np.uint64))
        assert np.array_equal(a["counters"], b["counters"])
    assert run_on[0][-1]["counters"].sum() > 0


def test_switch_off_exports_nothing(run_off, run_on):
    assert sum(len(r) for r in run_off[1]) == 0
    assert sum(len(r) for r in run_on[1]) >= 20


def test_blocking_and_deferred_runs_give_the_same_records(gpu_ctx, sim, run_on):
    snaps, recs, _ = _drive(gpu_ctx, sim, True, deferred=True)
    assert [len(r) for r in recs] == [len(r) for r in run_on[1]]
    a = np.concatenate(recs); b = np.concatenate(run_on[1])
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert np.array_equal(snaps[-1]["P"].view(np.uint64), run_on[0][-1]["P"].view(np.uint64))


def test_every_clone_that_leaves_the_window_is_exported_once_and_points_forward(run_on):
    snaps, recs, _ = run_on
    seen = []
    before = np.zeros(0, np.int64)
    for s, r in zip(snaps, recs):
        after = s["clones"]["id"]
        # the clones of the previous message that are gone now (a clone made and pruned within one message cannot happen: the newest
        # clone is never removed), in ascending id = pruning order
        left = np.array(sorted(set(before.tolist()) - set(after.tolist())), np.int64)
        assert np.array_equal(r["id"], left), (r["id"], left)
        assert np.all(np.isin(r["to_id"], after)) and np.all(r["to_id"] > r["id"]) and np.all(r["to_time"] > r["time"])
        for k in r:
            # the nearest newer survivor
            assert k["to_id"] == after[after > k["id"]].min()
            assert k["to_time"] == s["clones"]["time"][list(after).index(k["to_id"])]
        seen += r["id"].tolist(); before = after
    assert len(seen) == len(set(seen)) >= 20


def test_relative_pose_and_covariances_of_every_record(run_on):
    from tests.landmark_cov_ref import quat_to_rot
    snaps, recs, _ = run_on
    n = 0
    for s, r in zip(snaps, recs):
        for k in r:
            b = s["clones"][list(s["clones"]["id"]).index(k["to_id"])]      # nothing moves a clone between the export and the end of the message
            Ra, Rb = quat_to_rot(k["q"]), quat_to_rot(b["q"])
            assert np.max(np.abs(quat_to_rot(k["rel_q"]) - Ra.T @ Rb)) < 1e-12 and abs(np.linalg.norm(k["rel_q"]) - 1) < 1e-12
            assert np.max(np.abs(k["rel_p"] - Ra.T @ (b["p"] - k["p"]))) < 1e-12
            for S in (k["cov_abs"], k["cov_rel"]):
                assert np.all(np.isfinite(S)) and np.array_equal(S, S.T)
                assert np.linalg.eigvalsh(S).min() >= -1e-12 * np.trace(S)
            n += 1
    assert n >= 20


def test_window_covariance_against_the_restatement_on_the_same_instant(run_on):
    snaps, _, win = run_on
    worst = 0.0; n = 0
    for s, (ids, ca, cr) in list(zip(snaps, win))[::4]:
        cl = s["clones"]; P = s["P"]
        assert np.array_equal(ids, cl["id"]) and len(ids) >= 1
        assert np.all(np.isnan(cr[-1])) and np.all(np.isfinite(cr[:-1])) and np.all(np.isfinite(ca))
        for i in range(len(cl)):
            c = 22 + 6 * i
            assert np.array_equal(ca[i].view(np.uint64), np.ascontiguousarray(P[c:c + 6, c:c + 6]).view(np.uint64))
        for i in range(len(cl) - 1):
            S, err, _ = R.sigma_tracked(R.rel(R.clone_slot(cl[i], i), R.clone_slot(cl[i + 1], i + 1)), P)
            worst = max(worst, float(np.max(np.abs(cr[i].astype(R.LD) - S) / err))); n += 1
    print("get_window_cov: %d edges, worst |error| / bound %.3f" % (n, worst))
    assert n >= 50 and worst <= 1.0


def test_exported_relative_poses_lie_on_the_true_trajectory_as_their_covariance_says(sim, run_on):
    d2 = []
    for r in run_on[1]:
        for k in r:
            # the record's relative pose against the truth, through the error the covariance is stated for
            from tests.landmark_cov_ref import quat_to_rot
            qa0, pa0 = R.true_pose(sim["traj"], k["time"]); qb0, pb0 = R.true_pose(sim["traj"], k["to_time"])
            R0, t0 = R.rel_pose(qa0, pa0, qb0, pb0)
            e = np.concatenate([R.log_so3(R0 @ quat_to_rot(k["rel_q"].astype(R.LD)).T), t0 - k["rel_p"]]).astype(np.float64)
            d2.append(float(e @ np.linalg.solve(k["cov_rel"], e)))
    d2 = np.array(d2)
    q = np.quantile(d2, [0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
    print("%d records; d2 = e^T Sigma_rel^-1 e: 10/25/50/75/90/99 %% = %s, share below %.2f: %.3f" % (len(d2), np.array2string(q, precision=3), R.CHI2_6_999,
                                                                                                    np.mean(d2 < R.CHI2_6_999)))
    assert len(d2) >= 20 and np.median(d2) < R.CHI2_6_999


def test_a_transport_and_the_switch_refuse_each_other(gpu_ctx, sim):
    import ctypes as C
    import larvio_amd
    from larvio_amd._lib import LvkError
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 0)      # never called here
    fn = C.cast(cb, C.c_void_p)
    A = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert A.initialize()
    A.set_shard(0, 1, fn, None, keepalive=cb)
    with pytest.raises(LvkError) as ei:
        A.set_keyframe_export(True)
    assert "status 4" in str(ei.value) and "lvk_ekf_set_keyframe_export" in str(ei.value), str(ei.value)
    A.set_keyframe_export(False)                                         # off is always accepted
    A.close()
    B = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert B.initialize()
    B.set_keyframe_export(True)
    with pytest.raises(LvkError) as ei:
        B.set_shard(0, 1, fn, None, keepalive=cb)
    assert "status 4" in str(ei.value) and "keyframes" in str(ei.value), str(ei.value)
    B.close()
