"""GPU: position covariances of active and stable map points - the stage entry lvk_ekf_landmark_cov (k_landmark_cov), the filter's
getter lvk_ekf_get_feature_cov and the lost-point path (lvk_ekf_set_lost_feature_cov / lvk_ekf_take_lost_features_cov).
The reference is tests/landmark_cov_ref.py (long double; pinned on the CPU by tests/test_landmark_cov_ref.py); every comparison is
relative to the entrywise bound B = |J| |P_s| |J|^T."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import landmark_cov_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD
PAD = 3                                     # ldp = n + 3
# (n, L): 22 + two clones + one feature; 46 (IMU intrinsics in the state) + two clones + one feature
SHAPES = [(35, 22), (59, 46)]


def _jobs_for(n, L, first, count, seed):
    """job i anchors on clone (i + first) % 2 - the first and the last clone of the window - and reads the feature column n - 1, which
    with one in-state feature is the first and the last feature column at once"""
    rng = np.random.default_rng([seed, n, first])
    return np.array([R.random_job(rng, L + 6 * ((i + first) % 2), n - 1) for i in range(count)])


def _buffer(P, n, fill=np.nan):
    buf = np.full((n, n + PAD), fill)
    buf[:, :n] = P
    return buf


@functools.lru_cache(maxsize=None)
def _reference(n, L, first):
    """65 jobs on one random SPD covariance, with the restatement's Sigma, B and J: computed once per shape, shared by the job counts"""
    rng = np.random.default_rng([7, n, first])
    P = R.random_spd(rng, n)
    jobs = _jobs_for(n, L, first, 65, 1)
    ref = [R.sigma(j, P) for j in jobs]
    return P, jobs, ref


@pytest.mark.parametrize("n,L", SHAPES)
@pytest.mark.parametrize("n_jobs", [1, 2, 65])
@pytest.mark.parametrize("first", [0, 1])
def test_stage_entry_against_the_restatement(gpu_ctx, n, L, n_jobs, first):
    """random SPD P in a buffer of leading dimension n + 3 (NaN padding): Sigma within TOL_ND B of the restatement (central differences in
    long double), and exactly symmetric"""
    from larvio_amd import ops
    P, jobs, ref = _reference(n, L, first)
    got = ops.landmark_cov(gpu_ctx, _buffer(P, n), jobs[:n_jobs], n=n)
    assert got.shape == (n_jobs, 3, 3) and np.isfinite(got).all()
    worst = 0.0
    for k in range(n_jobs):
        S, B, _ = ref[k]
        assert np.array_equal(got[k], got[k].T)
        worst = max(worst, float(np.max(np.abs(got[k].astype(LD) - S) / B)))
    print("n %d jobs %d first anchor %d: worst |Sigma - restatement| / B = %.3g (TOL_ND %.3g)" % (n, n_jobs, first, worst, R.TOL_ND))
    assert worst <= R.TOL_ND


@pytest.mark.parametrize("n,L", SHAPES)
@pytest.mark.parametrize("n_jobs", [1, 2, 65])
@pytest.mark.parametrize("first", [0, 1])
def test_stage_entry_against_the_isotropic_closed_forms(gpu_ctx, n, L, n_jobs, first):
    """P_s block-diagonal with one isotropic block per error group (everything else of P random): Sigma is the sum of the closed forms,
    formed in long double without any differentiation; the kernel's 169 fp64 products per entry at 2^-53 each stay inside 1e-12 B with
    two orders of margin"""
    from larvio_amd import ops
    _, jobs, ref = _reference(n, L, first)
    rng = np.random.default_rng([9, n, first])
    s2 = rng.uniform(1e-6, 1e-3, 5)
    P = rng.normal(0, 1e-3, (n, n)); P = P + P.T
    cols = np.unique(np.concatenate([R.columns(j) for j in jobs[:n_jobs]]))
    P[np.ix_(cols, cols)] = 0.0
    for j in jobs[:n_jobs]:
        c = R.columns(j)
        P[c, c] = np.repeat(s2, [3, 3, 3, 3, 1])
    got = ops.landmark_cov(gpu_ctx, _buffer(P, n), jobs[:n_jobs], n=n)
    worst = 0.0
    for k in range(n_jobs):
        J = ref[k][2]
        B = R.bound(J, R.gather(P, jobs[k]))
        assert np.array_equal(got[k], got[k].T)
        worst = max(worst, float(np.max(np.abs(got[k].astype(LD) - R.sigma_closed(jobs[k], s2)) / B)))
    print("n %d jobs %d first anchor %d: worst |Sigma - closed forms| / B = %.3g" % (n, n_jobs, first, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("n,L", SHAPES)
@pytest.mark.parametrize("n_jobs", [1, 65])
def test_nothing_outside_the_13_rows_and_columns_is_read(gpu_ctx, n, L, n_jobs):
    """the same call with NaN in every entry of the P buffer that no job's 13 rows x 13 columns cover, padding columns included: the
    same bits as the clean run"""
    from larvio_amd import ops
    P, jobs, _ = _reference(n, L, 0)
    clean = ops.landmark_cov(gpu_ctx, _buffer(P, n, fill=0.25), jobs[:n_jobs], n=n)
    keep = np.zeros((n, n + PAD), bool)
    for j in jobs[:n_jobs]:
        c = R.columns(j)
        keep[np.ix_(c, c)] = True
    assert keep.sum() <= 2 * 169 - 49                  # two column sets sharing the extrinsics and the feature column
    buf = np.where(keep, _buffer(P, n), np.nan)
    got = ops.landmark_cov(gpu_ctx, buf, jobs[:n_jobs], n=n)
    assert np.isfinite(got).all() and np.array_equal(got, clean)


def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx):
    from larvio_amd import ops
    from larvio_amd._lib import lib, _p
    n, L = 35, 22
    P, jobs, _ = _reference(n, L, 0)
    buf = _buffer(P, n)
    good = ops.landmark_cov(gpu_ctx, buf, jobs[:2], n=n)
    Lb = lib(); dP = gpu_ctx.to_device(buf); out = np.full((2, 9), 7.0)
    ldp = n + PAD

    def call(d_P=dP, ld=ldp, nn=n, h_jobs=jobs[:2], n_jobs=2, h_out=out):
        hj = np.ascontiguousarray(h_jobs) if h_jobs is not None else None
        return Lb.lvk_ekf_landmark_cov(gpu_ctx.h, _p(d_P), ld, nn, _p(hj), n_jobs, _p(h_out))

    def edited(**kw):
        j = jobs[:2].copy()
        for k, v in kw.items():
            j[k][1] = v
        return j

    bad = [dict(d_P=None), dict(h_jobs=None), dict(h_out=None), dict(n_jobs=-1), dict(ld=n - 1),
           dict(h_jobs=edited(anchor_col=-1)), dict(h_jobs=edited(anchor_col=n - 5)), dict(h_jobs=edited(feat_col=-1)), dict(h_jobs=edited(feat_col=n)),
           dict(nn=20, ld=ldp), dict(h_jobs=edited(inv_depth=0.0))]
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(out == 7.0)                                     # nothing written
        assert b"lvk_ekf_landmark_cov" in Lb.lvk_last_error(gpu_ctx.h)
        assert np.array_equal(ops.landmark_cov(gpu_ctx, buf, jobs[:2], n=n), good)
    assert call(n_jobs=0) == 0 and np.all(out == 7.0)                  # LVK_OK, nothing to do
    assert call(h_jobs=edited(anchor_col=n - 6)) == 0                  # the last admissible anchor column


# ----------------------------------------------------------------------------------------------------------- the filter
def _drive(ctx, sim, lost_cov, per_message):
    """run the simulated messages (tests/feature_sim.py) through a fresh filter; per_message(gpu, updated) after each"""
    import larvio_amd
    gpu = larvio_amd.LarVio(sim["cfg"], ctx); assert gpu.initialize()
    if lost_cov is not None:
        gpu.set_lost_feature_cov(lost_cov)
    gpu.set_state(*sim["init"])
    imu = sim["imu"]; lo = 0
    for ts, m in sim["msgs"]:
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        upd, rest = gpu.processFeatures((ts, m), b)
        lo += len(b) - len(rest)
        per_message(gpu, upd)
    return gpu


def _snapshot(gpu):
    s = gpu.state()
    c = gpu.counters()
    ids, idp, pos = gpu.features()
    return dict(state=np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]]), P=gpu.cov(),
                ids=ids, idp=idp, pos=pos, clones=gpu.clones(), hybrid=c["hybrid"], counters=np.array([c[k] for k in sorted(c)]), R_b2c=s["R_b2c"], t_c_b=s["t_c_b"])


def _recover_obs(q_cam, p_cam, pos, rho):
    """the anchor observation (u, v) from the world position and the anchor camera pose: the inverse of the filter's
    p_w = R(q_cam) [u/rho, v/rho, 1/rho] + p_cam.  R(q_cam) is orthonormal only as far as the configured extrinsic rotation is (the
    quaternion it comes from is not normalised), so the system is solved, not multiplied by the transpose; and because the forward map
    rounds, the doubles next to that solution are tried and the pair that reproduces the position bit for bit (same operations in
    the same order as the filter's injection) is taken - the solution itself if none does."""
    Rc = R.quat_to_rot(np.asarray(q_cam, np.float64))
    d = np.linalg.solve(Rc, pos - p_cam)
    resid = ((pos - p_cam).astype(LD) - Rc.astype(LD) @ d.astype(LD)).astype(np.float64)
    dl = d.astype(LD) + np.linalg.solve(Rc, resid).astype(LD)                     # one step of refinement in long double
    u0, v0 = float(dl[0] / dl[2]), float(dl[1] / dl[2])

    def steps(x):
        out = [x]; lo = hi = x
        for _ in range(16):
            lo = np.nextafter(lo, -np.inf); hi = np.nextafter(hi, np.inf); out += [lo, hi]
        return out
    best = None; found = set()
    for u in steps(u0):
        for v in steps(v0):
            pc = (np.float64(u) / rho, np.float64(v) / rho, 1 / rho)
            pw = [Rc[i, 0] * pc[0] + Rc[i, 1] * pc[1] + Rc[i, 2] * pc[2] + p_cam[i] for i in range(3)]
            if pw[0] == pos[0] and pw[1] == pos[1] and pw[2] == pos[2]:
                found.add((float(u), float(v)))
                cost = abs(u - u0) + abs(v - v0)
                if best is None or cost < best[0]:
                    best = (cost, u, v)
    return (best[1], best[2], found) if best is not None else (u0, v0, found)


def _recover_obs_over_messages(history, fid, aid):
    """Several doubles (u, v) can round to the same position, and they do not give the same bits of Sigma.  The anchor observation stays
    what it is while the feature keeps its anchor, the position is refreshed with every injection: the pairs that reproduce the
    position after EVERY message of history (newest last) since the feature got this anchor are intersected."""
    cands = None; first = None
    for r in reversed(history):
        ids, anc, pos, _ = r["fc"]
        i = np.flatnonzero(ids == fid)
        if not len(i) or anc[int(i[0])] != aid:
            break
        i = int(i[0]); cl = r["snap"]["clones"]; k = int(np.flatnonzero(cl["id"] == aid)[0])
        u, v, found = _recover_obs(cl["q_cam"][k], cl["p_cam"][k], pos[i], np.float64(r["snap"]["idp"][i]))
        if first is None:
            first = (u, v)
        if found:
            cands = found if cands is None else ((cands & found) or cands)
            if len(cands) == 1:
                break
    if not cands:
        return first
    return min(cands, key=lambda c: abs(c[0] - first[0]) + abs(c[1] - first[1]))


def _rebuild_jobs(snap, ids, anchor_ids, pos, L=22, history=None):
    """the getter's jobs from what the public getters hand out; obs_anchor is recovered from the position and the anchor camera pose.
    -> (jobs, rows): rows = indices of the features whose anchor is in the window"""
    from larvio_amd.ops import LANDMARK_JOB
    cl = snap["clones"]; jobs = []; rows = []
    for i, (fid, aid) in enumerate(zip(ids, anchor_ids)):
        k = np.flatnonzero(cl["id"] == aid)
        if not len(k):
            continue
        k = int(k[0])
        j = np.zeros((), LANDMARK_JOB)
        j["anchor_col"] = L + 6 * k; j["feat_col"] = L + 6 * len(cl) + i
        j["q_anchor"] = cl["q"][k]; j["R_b2c"] = snap["R_b2c"].ravel(); j["t_c_b"] = snap["t_c_b"]
        j["inv_depth"] = snap["idp"][list(snap["ids"]).index(fid)]
        j["obs_anchor"] = (_recover_obs(cl["q_cam"][k], cl["p_cam"][k], pos[i], np.float64(j["inv_depth"]))[:2] if history is None
                           else _recover_obs_over_messages(history, fid, aid))
        jobs.append(j); rows.append(i)
    return np.array(jobs), rows


@pytest.fixture(scope="module")
def sim():
    from tests import feature_sim as F
    return F.simulate(4)


@pytest.fixture(scope="module")
def run_on(gpu_ctx, sim):
    """the stream with the switch on: a snapshot, get_feature_cov() and the lost points taken after every message"""
    rec = []

    def per_message(gpu, upd):
        rec.append(dict(upd=upd, snap=_snapshot(gpu), fc=gpu.get_feature_cov(), lost=gpu.take_lost_features_cov()))
    gpu = _drive(gpu_ctx, sim, True, per_message)
    gpu.close()
    return rec


@pytest.fixture(scope="module")
def run_off(gpu_ctx, sim):
    """the same stream with the switch off (the default is not touched): snapshots; the lost points are taken at the end"""
    rec = []
    gpu = _drive(gpu_ctx, sim, None, lambda g, upd: rec.append(dict(upd=upd, snap=_snapshot(g))))
    lost = gpu.take_lost_features_cov()
    gpu.close()
    return rec, lost


def _getter_case(run_on):
    """the last message after which a hybrid update has happened and at least 3 features are in the state"""
    pick = None
    for r in run_on:
        if r["snap"]["hybrid"] > 0 and len(r["fc"][0]) >= 3:
            pick = r
    assert pick is not None, "no message leaves a hybrid update behind with 3 features in the state"
    return pick


def test_getter_lists_the_features_of_get_features(run_on):
    n_checked = 0
    for r in run_on:
        ids, anc, pos, cov = r["fc"]
        assert np.array_equal(ids, r["snap"]["ids"]) and np.array_equal(pos, r["snap"]["pos"])
        assert cov.shape == (len(ids), 3, 3)
        for k in range(len(ids)):
            in_window = anc[k] in r["snap"]["clones"]["id"]
            assert np.isfinite(cov[k]).all() == in_window and (in_window or np.isnan(cov[k]).all())
            assert np.array_equal(cov[k], cov[k].T, equal_nan=True)
            n_checked += in_window
    assert n_checked >= 3


def test_getter_against_the_restatement(gpu_ctx, run_on):
    """the getter's Sigma against the restatement on jobs rebuilt from the public getters (obs_anchor recovered from the position: its
    rounding moves Sigma by a few ulp of B, far inside TOL_ND)"""
    r = _getter_case(run_on)
    ids, anc, pos, cov = r["fc"]
    jobs, rows = _rebuild_jobs(r["snap"], ids, anc, pos)
    assert len(rows) >= 3
    worst = 0.0
    for j, i in zip(jobs, rows):
        S, B, _ = R.sigma(j, r["snap"]["P"])
        worst = max(worst, float(np.max(np.abs(cov[i].astype(LD) - S) / B)))
    print("getter vs restatement: worst / B = %.3g over %d features" % (worst, len(rows)))
    assert worst <= R.TOL_ND


def test_getter_equals_the_stage_entry_bit_for_bit(gpu_ctx, run_on):
    """Jobs rebuilt in Python from get_cov, get_clones, get_state, get_features and the returned anchor ids, obs_anchor recovered from the
    position and the anchor camera pose, fed to the stage entry: the getter's Sigma must equal the stage entry's bit for bit.
    Both sides run the same kernel on the same covariance and columns, so only obs_anchor can tell them apart: the getter passes the
    filter's own anchor observation, the rebuilt job the one _recover_obs_over_messages finds (the doubles that reproduce the position
    bit for bit after every message since the feature got its anchor).
    MEASURED on an MI355X: with obs_anchor recovered through R(q_cam)^T, which is no inverse at the 4e-13 by which the configured
    extrinsic rotation misses orthonormality, 28 of 28 matrices differed (8.34e-12 B); with the system solved and the neighbouring
    doubles matched against the position of the one message, 5 of 28 (6.4e-16 B: several doubles give the same position).  The figures
    are printed before the assertion."""
    from larvio_amd import ops
    r = _getter_case(run_on)
    ids, anc, pos, cov = r["fc"]
    assert r["snap"]["hybrid"] > 0 and len(ids) >= 3                # lvk_ekf_counters[0]
    jobs, rows = _rebuild_jobs(r["snap"], ids, anc, pos, history=run_on[:[id(x) for x in run_on].index(id(r)) + 1])
    assert len(rows) >= 3
    stage = ops.landmark_cov(gpu_ctx, r["snap"]["P"], jobs)
    worst = 0.0; differ = 0
    for k, i in enumerate(rows):
        _, B, _ = R.sigma(jobs[k], r["snap"]["P"])
        worst = max(worst, float(np.max(np.abs(cov[i].astype(LD) - stage[k].astype(LD)) / B)))
        differ += not np.array_equal(cov[i], stage[k])
    print("getter vs stage entry on rebuilt jobs: %d of %d matrices differ in some bit, worst |diff| / B = %.3g" % (differ, len(rows), worst))
    assert differ == 0


def test_lost_points_carry_the_covariance_of_the_previous_message(gpu_ctx, run_on):
    """switch on: every point take_lost_features_cov() hands out carries the Sigma get_feature_cov() gave for its id after the previous
    message (propagation and augmentation leave the 13 rows and columns untouched: Phi's rows 9..21 are identity rows), within 1e-12 B"""
    n_lost = 0; worst = 0.0
    for prev, cur in zip(run_on[:-1], run_on[1:]):
        lid, lpos, lcov = cur["lost"]
        pids, panc, ppos, pcov = prev["fc"]
        for i, p, S in zip(lid, lpos, lcov):
            k = int(np.flatnonzero(pids == i)[0])                    # it was in the state after the previous message
            assert np.abs(p - ppos[k]).max() < 1e-9
            if not np.isfinite(pcov[k]).all():
                assert np.isnan(S).all()
                continue
            jobs, rows = _rebuild_jobs(prev["snap"], pids[k:k + 1], panc[k:k + 1], ppos[k:k + 1])
            jobs["feat_col"] += k                                    # _rebuild_jobs numbered the slice from 0
            _, B, _ = R.sigma(jobs[0], prev["snap"]["P"])
            assert np.array_equal(S, S.T)
            worst = max(worst, float(np.max(np.abs(S.astype(LD) - pcov[k].astype(LD)) / B)))
            n_lost += 1
    print("lost points with a covariance: %d, worst |Sigma_lost - Sigma_previous| / B = %.3g" % (n_lost, worst))
    assert n_lost >= 3
    assert worst <= 1e-12


def test_switch_off_gives_nan_covariances_and_the_positions_of_take_lost_features(gpu_ctx, sim, run_off):
    _, (ids, pos, cov) = run_off
    assert len(ids) >= 3 and np.isnan(cov).all()
    gpu = _drive(gpu_ctx, sim, None, lambda g, upd: None)
    ids2, pos2 = gpu.stable_map_points()
    gpu.close()
    assert np.array_equal(ids, ids2) and np.array_equal(pos, pos2)


def test_switch_has_no_side_effect_on_the_filter(run_on, run_off):
    """the same stream with the switch on and off: state, full covariance, in-state ids and counters equal after every update"""
    off, lost_off = run_off
    assert len(off) == len(run_on) and sum(r["upd"] for r in off) >= 50
    for a, b in zip(run_on, off):
        assert a["upd"] == b["upd"]
        for k in ("state", "P", "ids", "counters", "idp", "pos"):
            assert np.array_equal(a["snap"][k], b["snap"][k]), k
    lost_on = [r["lost"] for r in run_on]
    assert np.array_equal(np.concatenate([l[0] for l in lost_on]), lost_off[0])
    assert np.array_equal(np.concatenate([l[1] for l in lost_on]), lost_off[1])
