"""lvk_ekf_update_landmarks (k_lm_rows, k_lm_gain, k_lm_downdate, be_landmark_fix.hip) against the long-double restatement
tests/landmark_fix_ref.py, inside the componentwise bound derived there: n_obs = 1, 5, 6, 7 (12 rows: the compression edge), 63 / 64 /
65, 256 / 257, 1024; n = 28 (clone_col 22: the last six columns), 216 and 433, ldp = n and padded; the clone first, in the middle and
last in the window (landmark_fix_ref.stage_problems); per-observation status identical; exact symmetry; repeatability, also under a
permutation of the observations; NaN in everything the call must not read; rejected observations and rejected batches; every refusal.

Under a permutation the per-observation outputs (status, gamma_k) are the same bits, permuted; dx, P and the batch's gamma of a
compressed batch depend on the order of the rows as any QR does, and both orders are held to the restatement's bound - which is 1e-2
of dx and less (tests/test_landmark_fix_ref.py): the compression keeps as many rows as the system has rank, and none of rounding noise."""
import numpy as np
import pytest

from tests import landmark_fix_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _run(ctx, pr, obs=None, P=None, **job_kw):
    from larvio_amd import ops
    return ops.update_landmarks(ctx, R.buffer(pr["P"], pr["n"], pr["ldp"]) if P is None else P, R.job_record(pr["job"], **job_kw), pr["obs"] if obs is None else obs, n=pr["n"])


@pytest.fixture(scope="module")
def problems():
    return R.stage_tracked()


@pytest.fixture(scope="module")
def results(gpu_ctx, problems):
    return [_run(gpu_ctx, pr) for pr, _ in problems]


def _same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_stage_entry_against_the_restatement_within_the_derived_bound(problems, results):
    worst = {}
    for (pr, t), (dx, Pb, info, st, gam) in zip(problems, results):
        n = pr["n"]
        assert np.array_equal(st, t["status"]), pr["name"]
        assert [int(x) for x in info[3:8]] == [t["n_used"], t["n_gated"], t["n_behind"], t["m"], 0] and int(info[0]) == t["batch_status"] == 0, (pr["name"], info)
        assert np.all(np.isfinite(dx)) and np.all(np.isfinite(Pb[:, :n])) and np.all(np.isnan(Pb[:, n:])) and np.all(np.isfinite(gam))
        assert np.all(gam[st == R.BEHIND] == 0)
        live = st != R.BEHIND
        wg = R.worst_ratio(gam[live].astype(LD) - t["gamma"][live], t["e_gamma"][live])
        wb = float(abs(LD(info[1]) - t["gamma_b"]) / t["e_gamma_b"])
        assert abs(LD(info[2]) - t["pmin"]) <= 1e-6 * abs(t["pmin"])
        wd = R.worst_ratio(dx.astype(LD) - t["dx"], t["e_dx"]); wp = R.worst_ratio(Pb[:, :n].astype(LD) - t["P"], t["e_P"])
        print("%-18s n %3d ldp %3d n_obs %4d used %4d m %2d: worst |error| / bound dx %.4f P %.4f gamma_k %.4f batch gamma %.4f" %
              (pr["name"], n, pr["ldp"], len(pr["obs"]), t["n_used"], t["m"], wd, wp, wg, wb))
        key = "n_used <= 6" if t["n_used"] <= 6 else "compressed"
        w = worst.setdefault(key, dict(dx=0.0, P=0.0, gamma_k=0.0, gamma=0.0))
        w["dx"] = max(w["dx"], wd); w["P"] = max(w["P"], wp); w["gamma_k"] = max(w["gamma_k"], wg); w["gamma"] = max(w["gamma"], wb)
    print("worst |error| / bound per group:", worst)
    assert max(max(w.values()) for w in worst.values()) <= 1.0


def test_P_is_exactly_symmetric_and_two_calls_give_the_same_bits(gpu_ctx, problems, results):
    for (pr, _), res in zip(problems, results):
        n = pr["n"]
        assert _same_bits(pr["P"], pr["P"].T)
        assert _same_bits(res[1][:, :n], res[1][:, :n].T), pr["name"]
        again = _run(gpu_ctx, pr)
        assert all(_same_bits(a, b) for a, b in zip(res, again)), pr["name"]


def test_permuted_observations_give_the_same_bits_per_observation(gpu_ctx, problems, results):
    for k in (3, 7, 8, 11):
        (pr, t), (dx, Pb, info, st, gam) = problems[k], results[k]
        perm = np.random.default_rng(k).permutation(len(pr["obs"]))
        dx2, Pb2, info2, st2, gam2 = _run(gpu_ctx, pr, obs=pr["obs"][perm])
        assert np.array_equal(st2, st[perm]) and _same_bits(gam2, gam[perm]), pr["name"]
        assert _same_bits(info2[3:], info[3:])
        n = pr["n"]
        assert R.worst_ratio(dx2.astype(LD) - t["dx"], t["e_dx"]) <= 1.0 and R.worst_ratio(Pb2[:, :n].astype(LD) - t["P"], t["e_P"]) <= 1.0
        assert abs(LD(info2[1]) - t["gamma_b"]) <= t["e_gamma_b"], pr["name"]


def test_nan_in_everything_unread_before_the_gain_step_changes_nothing_when_all_is_gated(gpu_ctx, problems):
    """every entry of P outside the twelve rows AND columns is NaN, the padding too; the batch is gated out to the last observation (all
    observations moved 1e4 off in the image under the filter's own gate): not one byte changes"""
    for k in (3, 9):                                    # n = 28 with ldp = n + 5, n = 433 with ldp = n
        pr, _ = problems[k]
        n = pr["n"]; cols = R.columns(pr["job"])
        buf = np.full((n, pr["ldp"]), np.nan); buf[np.ix_(cols, cols)] = pr["P"][np.ix_(cols, cols)]
        obs = pr["obs"].copy(); obs["uv"] += 1e4
        dx, Pb, info, st, gam = _run(gpu_ctx, pr, obs=obs, P=buf, gate=R.CHI2_005_2)
        assert np.all(st == R.GATED) and int(info[0]) == 1 and [int(x) for x in info[3:7]] == [0, len(obs), 0, 0]
        assert np.all(dx == 0) and Pb.tobytes() == buf.tobytes(), pr["name"]
        # the lower triangle of cov_w is not read either
        o2 = pr["obs"].copy(); o2["cov_w"][:, [3, 6, 7]] = np.nan
        res = _run(gpu_ctx, pr, obs=o2); ref = _run(gpu_ctx, pr)
        assert all(_same_bits(a, b) for a, b in zip(res, ref))


def test_a_mixed_batch_equals_the_batch_of_its_used_observations_bit_for_bit(gpu_ctx, problems, results):
    n_checked = 0
    for (pr, t), (dx, Pb, info, st, gam) in zip(problems, results):
        if not pr["mixed"]:
            continue
        assert t["n_used"] and t["n_gated"] + t["n_behind"], pr["name"]
        used = st == R.USED
        dx2, Pb2, info2, st2, gam2 = _run(gpu_ctx, pr, obs=pr["obs"][used])
        assert np.all(st2 == R.USED) and _same_bits(gam2, gam[used])
        assert _same_bits(dx, dx2) and _same_bits(Pb, Pb2) and _same_bits(info[:3], info2[:3]) and info2[3] == info[3] and info2[6] == info[6], pr["name"]
        n_checked += 1
    assert n_checked >= 3


def test_all_gated_and_all_behind_batches_leave_every_byte_of_P(gpu_ctx, problems):
    for k in (1, 5, 10):
        pr, _ = problems[k]
        before = R.buffer(pr["P"], pr["n"], pr["ldp"])
        obs = pr["obs"].copy(); obs["uv"] += 1e4
        dx, Pb, info, st, gam = _run(gpu_ctx, pr, obs=obs, gate=R.CHI2_005_2)
        assert np.all(st == R.GATED) and np.all(gam > R.CHI2_005_2) and int(info[0]) == 1 and info[1] == 0 and np.all(dx == 0) and Pb.tobytes() == before.tobytes()
        # behind: the camera turned round (R_b2c -> diag(-1, 1, -1) R_b2c)
        Rback = (np.diag([-1.0, 1.0, -1.0]) @ pr["job"]["R_b2c"]).ravel()
        dx, Pb, info, st, gam = _run(gpu_ctx, pr, R_b2c=Rback)
        assert np.all(st == R.BEHIND) and np.all(gam == 0) and int(info[0]) == 1 and [int(x) for x in info[3:7]] == [0, 0, len(obs), 0]
        assert np.all(dx == 0) and Pb.tobytes() == before.tobytes()
        # min_depth far beyond every point: all behind, nothing divided
        dx, Pb, info, st, gam = _run(gpu_ctx, pr, min_depth=1e6)
        assert np.all(st == R.BEHIND) and np.all(np.isfinite(gam)) and Pb.tobytes() == before.tobytes()


def test_refusals_launch_nothing_and_leave_the_context_usable(gpu_ctx, problems, results):
    import ctypes as C
    from larvio_amd._lib import lib, _p
    from larvio_amd.ops import LANDMARK_OBS
    k = 7                                                                    # n = 216, padded, 40 observations, mixed
    (pr, _), good = problems[k], results[k]
    n = pr["n"]; no = len(pr["obs"])
    Lb = lib(); dP = gpu_ctx.to_device(R.buffer(pr["P"], n, pr["ldp"]))
    dx = np.full(n, 7.0); info = np.full(8, 7.0); st = np.full(1025, 7, np.int32); gam = np.full(1025, 7.0)
    vp, i = C.c_void_p, C.c_int
    Lb.lvk_ekf_update_landmarks.argtypes = [vp, vp, i, i, vp, vp, i, vp, vp, vp, vp]; Lb.lvk_ekf_update_landmarks.restype = i
    job = R.job_record(pr["job"]); obs = np.ascontiguousarray(pr["obs"], LANDMARK_OBS)

    def call(d_P=dP, ld=pr["ldp"], nn=n, j=job, o=obs, k_obs=None, h_dx=dx, h_info=info, h_st=st, h_g=gam, ctx=gpu_ctx.h):
        ptr = lambda a: None if a is None else _p(a)
        return Lb.lvk_ekf_update_landmarks(ctx, ptr(d_P), ld, nn, ptr(j), ptr(o), (no if o is None else len(o)) if k_obs is None else k_obs, ptr(h_dx), ptr(h_info), ptr(h_st), ptr(h_g))

    def job_with(**kw):
        return R.job_record(pr["job"], **kw)

    def obs_with(idx, key, v):
        o = obs.copy(); o[key][idx] = v
        return o
    not_psd = np.array([1.0, 2, 0, 2, 1, 0, 0, 0, 1]); neg = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, -1e-9])
    bad = [dict(d_P=None), dict(j=None), dict(o=None), dict(h_dx=None), dict(h_info=None), dict(h_st=None), dict(h_g=None), dict(ld=n - 1),
           dict(j=job_with(clone_col=20)), dict(j=job_with(clone_col=n - 5)), dict(j=job_with(q_b=pr["job"]["q_b"] * 1.00001)),
           dict(j=job_with(q_b=np.array([np.nan, 0, 0, 1]))), dict(j=job_with(p_b=np.array([0, np.inf, 0]))), dict(j=job_with(t_c_b=np.array([0, 0, np.nan]))),
           dict(j=job_with(R_b2c=np.full(9, np.nan))), dict(j=job_with(gate=np.nan)), dict(j=job_with(min_depth=-0.1)), dict(j=job_with(min_depth=np.nan)),
           dict(o=obs_with(3, "p_w", np.array([0, np.nan, 0]))), dict(o=obs_with(no - 1, "uv", np.array([np.inf, 0]))), dict(o=obs_with(0, "sigma", 0.0)),
           dict(o=obs_with(5, "sigma", -1e-3)), dict(o=obs_with(5, "sigma", np.nan)), dict(o=obs_with(2, "cov_w", not_psd)), dict(o=obs_with(2, "cov_w", neg)),
           dict(o=obs_with(9, "cov_w", np.array([1.0, np.nan, 0, 0, 1, 0, 0, 0, 1])))]
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(dx == 7.0) and np.all(info == 7.0) and np.all(st == 7) and np.all(gam == 7.0)              # nothing written
        assert b"lvk_ekf_update_landmarks" in Lb.lvk_last_error(gpu_ctx.h)
    big = np.zeros(1025, LANDMARK_OBS); big[:] = obs[0]
    assert call(o=big) == 3 and np.all(dx == 7.0)                     # LVK_ERR_CAPACITY
    assert call(k_obs=0) == 0 and np.all(dx == 7.0) and np.all(info == 7.0)      # an empty batch: LVK_OK, nothing launched or written
    assert call(ctx=None) == 1
    assert gpu_ctx.to_host(dP, np.float64, (n, pr["ldp"])).tobytes() == R.buffer(pr["P"], n, pr["ldp"]).tobytes()      # P untouched by all of them
    assert call() == 0                                                 # ... and the context is usable
    assert _same_bits(dx, good[0]) and _same_bits(info, good[2]) and np.array_equal(st[:no], good[3]) and _same_bits(gam[:no], good[4])
    assert _same_bits(gpu_ctx.to_host(dP, np.float64, (n, pr["ldp"])), good[1])
