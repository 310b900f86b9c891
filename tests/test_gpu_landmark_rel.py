"""lvk_ekf_get_feature_rel on simulated messages (tests/feature_sim.py, sw_size 10, the 41 messages of tests/test_gpu_keyframes.py): the
getter is a pure observer (state, covariance and counters keep their bits), lists the features of lvk_ekf_get_features, equals the
stage entry lvk_ekf_landmark_rel_cov on jobs rebuilt from the public getters, sits inside the restatement's bound
(tests/landmark_rel_ref.py) on the covariance of that instant, gives the same bits in blocking and deferred runs, refuses a clone id
that is not in the window, and returns symmetric, positive semi-definite matrices.

The newest clone against the IMU state (to_clone_id = newest id against -1): the augmentation copies the IMU pose into the new clone, but
the update then corrects the two through their own columns of the gain and a pruning update may follow, so inject() does not promise
that the two poses keep the same bits; test_newest_clone_and_imu_state_as_targets compares them where they do coincide and states the
difference where they do not."""
import numpy as np
import pytest

from tests import landmark_rel_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _bytes(t):
    return b"".join(np.ascontiguousarray(x).tobytes() for x in t)


def _drive(ctx, sim, getter, deferred=False):
    """-> one record per message: snapshot (state, covariance, counters, features, clones) and, with getter, get_feature_cov() and
    get_features_in_camera() for the IMU state and for the newest clone"""
    import larvio_amd
    from tests.test_gpu_landmark_cov import _snapshot
    gpu = larvio_amd.LarVio(sim["cfg"], ctx); assert gpu.initialize()
    gpu.set_state(*sim["init"])
    imu = sim["imu"]; lo = 0; rec = []
    for ts, m in sim["msgs"]:
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = (gpu.processFeaturesAsync if deferred else gpu.processFeatures)((ts, m), b)
        lo += len(b) - len(rest)
        r = {}
        if getter:
            r["rel"] = gpu.get_features_in_camera()
            cl = gpu.clones()
            r["rel_new"] = gpu.get_features_in_camera(int(cl["id"][-1])) if len(cl) else None
            r["fc"] = gpu.get_feature_cov()
        r["snap"] = _snapshot(gpu)
        rec.append(r)
    if getter:
        with pytest.raises(larvio_amd.LvkError, match="lvk_ekf_get_feature_rel"):
            gpu.get_features_in_camera(10 ** 12)                               # no such clone: refused ...
        again = gpu.get_features_in_camera()
        assert _bytes(again) == _bytes(rec[-1]["rel"])                        # ... and the next call works
    gpu.close()
    return rec


@pytest.fixture(scope="module")
def sim():
    from tests import feature_sim as F
    return F.simulate(4, t1=6.0, sw_size=10, fresh_ids=True)


@pytest.fixture(scope="module")
def run_on(gpu_ctx, sim):
    return _drive(gpu_ctx, sim, True)


@pytest.fixture(scope="module")
def run_off(gpu_ctx, sim):
    return _drive(gpu_ctx, sim, False)


def test_getter_has_no_side_effect_on_the_filter(run_on, run_off):
    assert len(run_on) == len(run_off) >= 40
    for a, b in zip(run_on, run_off):
        for k in ("state", "P", "ids", "counters", "idp", "pos"):
            assert a["snap"][k].shape == b["snap"][k].shape and a["snap"][k].tobytes() == b["snap"][k].tobytes(), k
    assert run_on[-1]["snap"]["counters"].sum() > 0


def test_getter_lists_the_features_of_get_features(run_on):
    n = 0
    for r in run_on:
        ids, anc, pos, cov = r["rel"]
        assert np.array_equal(ids, r["snap"]["ids"]) and np.array_equal(ids, r["fc"][0]) and np.array_equal(anc, r["fc"][1])
        assert pos.shape == (len(ids), 3) and cov.shape == (len(ids), 3, 3)
        for k in range(len(ids)):
            in_window = anc[k] in r["snap"]["clones"]["id"]
            assert np.isfinite(cov[k]).all() == in_window and np.isfinite(pos[k]).all() == in_window
            assert in_window or (np.isnan(cov[k]).all() and np.isnan(pos[k]).all())
            n += in_window
    assert n >= 100


def test_every_sigma_is_symmetric_and_positive_semidefinite(run_on):
    n = 0; least = np.inf
    for r in run_on:
        for rel in (r["rel"], r["rel_new"]):
            for S in rel[3]:
                if not np.isfinite(S).all():
                    continue
                assert np.array_equal(S.view(np.uint64), np.ascontiguousarray(S.T).view(np.uint64))
                ev = float(np.linalg.eigvalsh(S).min()) / float(np.trace(S)); least = min(least, ev)
                assert ev >= -1e-12
                n += 1
    print("%d matrices, smallest eigenvalue / trace %.3g" % (n, least))
    assert n >= 200


def _case(run_on):
    """(index, record) of the last message after which a hybrid update has happened and at least 3 features are in the state"""
    pick = None
    for i, r in enumerate(run_on):
        if r["snap"]["hybrid"] > 0 and len(r["rel"][0]) >= 3:
            pick = (i, r)
    assert pick is not None
    return pick


def _rebuilt(gpu_ctx, run_on, i, r, to_new):
    """LANDMARK_REL_JOB records of message i rebuilt from the public getters, for the features whose anchor observation the recovery of
    tests/test_gpu_landmark_cov.py finds EXACTLY: that is checked independently of the code under test, by the world-frame stage entry
    lvk_ekf_landmark_cov giving the bits of lvk_ekf_get_feature_cov on the rebuilt job.  -> (records, rows)"""
    from larvio_amd import ops
    from tests.test_gpu_landmark_cov import _rebuild_jobs
    snap = r["snap"]; ids, anc, pos, cov = r["fc"]
    wj, rows = _rebuild_jobs(snap, ids, anc, pos, history=run_on[:i + 1])
    world = ops.landmark_cov(gpu_ctx, snap["P"], wj)
    exact = [k for k, row in enumerate(rows) if np.array_equal(world[k].view(np.uint64), cov[row].view(np.uint64))]
    print("anchor observation recovered exactly for %d of %d features" % (len(exact), len(rows)))
    cl = snap["clones"]; s = snap["state"]
    rec = np.zeros(len(exact), ops.LANDMARK_REL_JOB)
    for o, k in enumerate(exact):
        for name in ops.LANDMARK_JOB.names:
            rec[o][name] = wj[k][name]
        ka = (int(wj[k]["anchor_col"]) - 22) // 6
        rec[o]["p_anchor"] = cl["p"][ka]
        if to_new:
            kb = len(cl) - 1
            rec[o]["b_theta_col"] = 22 + 6 * kb; rec[o]["b_p_col"] = 25 + 6 * kb; rec[o]["q_b"] = cl["q"][kb]; rec[o]["p_b"] = cl["p"][kb]
        else:
            rec[o]["b_theta_col"] = 0; rec[o]["b_p_col"] = 6; rec[o]["q_b"] = s[1:5]; rec[o]["p_b"] = s[8:11]
    return rec, [rows[k] for k in exact]


@pytest.mark.parametrize("to_new", (False, True))
def test_getter_equals_the_stage_entry_and_sits_inside_the_restatements_bound(gpu_ctx, run_on, to_new):
    from larvio_amd import ops
    i, r = _case(run_on)
    rec, rows = _rebuilt(gpu_ctx, run_on, i, r, to_new)
    assert len(rows) >= 3
    ids, anc, pos, cov = r["rel_new"] if to_new else r["rel"]
    pc, S = ops.landmark_rel_cov(gpu_ctx, r["snap"]["P"], rec)
    assert np.array_equal(pc.view(np.uint64), np.ascontiguousarray(pos[rows]).view(np.uint64))
    assert np.array_equal(S.view(np.uint64), np.ascontiguousarray(cov[rows]).view(np.uint64))
    worst = 0.0
    for j, row in zip(R.unpack(rec), rows):
        pc0, err_p, S0, err, Bnd = R.tracked(j, r["snap"]["P"])
        worst = max(worst, float(np.max(np.abs(pos[row].astype(LD) - pc0) / err_p)), float(np.max(np.abs(cov[row].astype(LD) - S0) / err)))
    print("getter (%s) vs restatement on cov(): worst |error| / bound %.3f over %d features" % ("newest clone" if to_new else "IMU state", worst, len(rows)))
    assert worst <= 1.0


def test_blocking_and_deferred_runs_agree_bit_for_bit(gpu_ctx, sim, run_on):
    d = _drive(gpu_ctx, sim, True, deferred=True)
    assert len(d) == len(run_on)
    for a, b in zip(d, run_on):
        assert _bytes(a["rel"]) == _bytes(b["rel"]) and _bytes(a["rel_new"]) == _bytes(b["rel_new"])
        assert a["snap"]["P"].tobytes() == b["snap"]["P"].tobytes()


def test_newest_clone_and_imu_state_as_targets(run_on):
    """Where the newest clone's pose has the bits of the IMU state's, the kernel forms the same p_c and the same J for the two targets
    (the same operations on the same numbers): p_c has the same bits, and the two Sigma differ by J (P_s,new - P_s,imu) J^T - the clone's
    columns of P against the IMU state's - plus each one's rounding, i.e. by at most bound_new + bound_imu + |J| |P_s,new - P_s,imu| |J|^T.
    Where the poses differ, the difference is stated."""
    same = differ = 0; worst = 0.0; dq = dp = 0.0
    for r in run_on:
        s = r["snap"]["state"]; cl = r["snap"]["clones"]; P = r["snap"]["P"]
        if not len(cl):
            continue
        if np.array_equal(cl["q"][-1], s[1:5]) and np.array_equal(cl["p"][-1], s[8:11]):
            same += 1
            ok = np.isfinite(r["rel"][3]).all(axis=(1, 2))
            assert np.array_equal(r["rel"][2][ok], r["rel_new"][2][ok])
            st = dict(q=s[1:5], p=s[8:11], R_b2c=s[17:26], t_c_b=s[26:29])
            ji, rows = R.filter_jobs(st, cl, r["rel"][0], r["snap"]["idp"], r["snap"]["pos"], anchor_ids=r["rel"][1])
            jn, _ = R.filter_jobs(st, cl, r["rel"][0], r["snap"]["idp"], r["snap"]["pos"], anchor_ids=r["rel"][1], to_clone_id=int(cl["id"][-1]))
            for a, b, row in list(zip(ji, jn, rows))[:4]:
                J = np.abs(R.jacobian_closed(a))
                allow = R.tracked(a, P)[3] + R.tracked(b, P)[3] + J @ np.abs(R.gather(P, b) - R.gather(P, a)) @ J.T
                w = float(np.max(np.abs(r["rel"][3][row].astype(LD) - r["rel_new"][3][row].astype(LD)) / allow)); worst = max(worst, w)
                assert w <= 1.0
        else:
            differ += 1
            dq = max(dq, float(np.max(np.abs(cl["q"][-1] - s[1:5])))); dp = max(dp, float(np.max(np.abs(cl["p"][-1] - s[8:11]))))
    print("newest clone == IMU state after %d messages, not after %d (largest |dq| %.3g, |dp| %.3g m); where equal: worst |Sigma_new - Sigma_imu| / allowance %.3g"
          % (same, differ, dq, dp, worst))
    assert same + differ >= 40
