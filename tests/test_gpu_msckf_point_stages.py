"""lvk_ekf_msckf_point_cov (k_msckf_point_cov, be_msckf_point.hip) against the long-double restatement tests/msckf_point_ref.py, inside
the componentwise bound derived there: M = 2, 3, 31, 32, 33, 62, 63, 64, leg_dim 22 / 46, estimate_td, if_fej, n from leg_dim + 6 M
to 433, ldp = n and padded, 1 / 7 / 300 jobs, ranks descending and scattered (msckf_point_ref.stage_launches); the two closed forms;
NaN everywhere outside P[cc, cc]; a degenerate job among good ones; exact symmetry; repeatability; every refusal."""
import numpy as np
import pytest

from tests import msckf_point_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _run(ctx, L, P=None, probs=None):
    from larvio_amd import ops
    probs = L["probs"] if probs is None else probs
    jobs, rk, z, zv = R.pack(probs)
    buf = R.buffer(L["P"] if P is None else P, L["n"], L["ldp"])
    return ops.msckf_point_cov(ctx, buf, L["clones"], jobs, rk, z, zv, leg_dim=L["leg_dim"], if_fej=L["if_fej"], estimate_td=L["estimate_td"], sigma2=L["sigma2"], n=L["n"])


@pytest.fixture(scope="module")
def launches():
    """every launch with its reference: (Sigma, bound, Bnd) per job, computed once"""
    out = []
    for L in R.stage_launches():
        ref = [R.sigma_tracked(pr, L["P"])[:3] for pr in L["probs"]]
        out.append((L, ref))
    return out


@pytest.fixture(scope="module")
def results(gpu_ctx, launches):
    return [_run(gpu_ctx, L) for L, _ in launches]


def test_stage_entry_against_the_restatement_within_the_derived_bound(launches, results):
    worst = 0.0; worst_b = 0.0
    for (L, ref), (got, ok) in zip(launches, results):
        assert np.all(ok == 1), L["name"]
        w = 0.0
        for k, (S, err, Bnd) in enumerate(ref):
            d = np.abs(got[k].astype(LD) - S)
            w = max(w, float(np.max(d / err))); worst_b = max(worst_b, float(np.max(d / Bnd)))
        print("%-9s n %3d ldp %3d leg %2d td %d fej %d jobs %3d: worst |error| / bound %.3f" % (L["name"], L["n"], L["ldp"], L["leg_dim"], L["estimate_td"], L["if_fej"],
                                                                                              len(ref), w))
        worst = max(worst, w)
    print("worst |error| / bound %.3f, worst |error| / Bnd %.3g" % (worst, worst_b))
    assert worst <= 1.0


def test_sigma_is_exactly_symmetric_and_two_calls_give_the_same_bits(gpu_ctx, launches, results):
    for (L, _), (got, ok) in zip(launches, results):
        assert np.array_equal(got, np.swapaxes(got, 1, 2))
        again, ok2 = _run(gpu_ctx, L)
        assert np.array_equal(again.view(np.uint64), got.view(np.uint64)) and np.array_equal(ok, ok2)


def test_nothing_of_P_outside_cc_is_read(gpu_ctx, launches, results):
    for (L, _), (got, ok) in zip(launches, results):
        if len(L["probs"]) > 7:
            continue
        for k, pr in enumerate(L["probs"]):
            cc = R.columns(pr["ranks"], L["leg_dim"])
            keep = np.zeros((L["n"], L["n"]), bool); keep[np.ix_(cc, cc)] = True
            one, ok1 = _run(gpu_ctx, L, P=np.where(keep, L["P"], np.nan), probs=[pr])
            assert ok1[0] == 1 and np.array_equal(one[0].view(np.uint64), got[k].view(np.uint64)), (L["name"], k)


def test_zero_state_covariance_gives_the_pixel_noise_term(gpu_ctx, launches):
    for L, _ in launches[:8]:
        Z = np.zeros_like(L["P"])
        got, ok = _run(gpu_ctx, L, P=Z)
        for k, pr in enumerate(L["probs"]):
            S, err, Bnd, _ = R.sigma_tracked(pr, Z)
            assert ok[k] == 1 and np.all(np.abs(got[k].astype(LD) - S) <= err), (L["name"], k)


def test_common_position_error_adds_s2_identity(gpu_ctx, launches):
    """position blocks of a job's observing clones at s2 I, fully correlated: Sigma = sigma2 A^-1 + s2 I (each job in its own launch:
    the covariance is the job's)"""
    s2 = 2.5e-3
    for L, _ in launches[:8]:
        pr = L["probs"][0]
        P = R.correlated_position_cov(L["n"], pr["ranks"], L["leg_dim"], s2)
        got, ok = _run(gpu_ctx, L, P=P, probs=[pr])
        got0, _ = _run(gpu_ctx, L, P=0 * P, probs=[pr])
        S, err, Bnd, _ = R.sigma_tracked(pr, P)
        _, err0, _, _ = R.sigma_tracked(pr, 0 * P)
        assert ok[0] == 1 and np.all(np.abs(got[0].astype(LD) - S) <= err)
        # ... and directly: the difference of the two device results is s2 I within the two bounds
        assert np.all(np.abs((got[0] - got0[0]).astype(LD) - LD(s2) * np.eye(3, dtype=LD)) <= err + err0 + R.U * np.abs(got[0]))


def test_a_degenerate_job_gets_nans_and_leaves_its_neighbours_alone(gpu_ctx):
    from larvio_amd import ops
    rng = np.random.default_rng(11)
    clones = R.make_clones(rng, 8)
    deg = R.degenerate_problem(4)
    clones[4:8] = deg["clones"]                        # ranks 4..7: four clones with one pose
    deg = dict(deg, clones=clones, ranks=[4, 5, 6, 7])
    good = [R.make_problem(rng, clones, [3, 1, 0]), R.make_problem(rng, clones, [0, 2, 3, 1])]
    n = 22 + 6 * 8; P = R.random_spd(rng, n)
    L = dict(clones=clones, P=P, n=n, ldp=n, leg_dim=22, if_fej=0, estimate_td=0, sigma2=good[0]["sigma2"])
    got, ok = _run(gpu_ctx, L, probs=[good[0], deg, good[1]])
    alone, ok_alone = _run(gpu_ctx, L, probs=good)
    assert list(ok) == [1, 0, 1] and np.all(np.isnan(got[1]))
    assert np.array_equal(got[[0, 2]].view(np.uint64), alone.view(np.uint64)) and np.all(ok_alone == 1)
    for k, pr in ((0, good[0]), (2, good[1])):
        S, err, _, _ = R.sigma_tracked(pr, P)
        assert np.all(np.abs(got[k].astype(LD) - S) <= err)


def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx, launches, results):
    from larvio_amd._lib import lib, _p
    from larvio_amd.larvio import CLONE
    L, _ = launches[1]; good, _ = results[1]                                   # M = 3, 7 jobs
    jobs, rk, z, zv = R.pack(L["probs"])
    buf = R.buffer(L["P"], L["n"], L["ldp"]); n = L["n"]
    Lb = lib(); dP = gpu_ctx.to_device(buf)
    clones = np.ascontiguousarray(L["clones"], CLONE)
    out = np.full((len(jobs), 9), 7.0); okw = np.full(len(jobs), 7, np.int32)
    import ctypes as C
    vp, i = C.c_void_p, C.c_int
    Lb.lvk_ekf_msckf_point_cov.argtypes = [vp, vp, i, i, vp, i, vp, i, vp, vp, vp, i, i, i, C.c_double, vp, vp]; Lb.lvk_ekf_msckf_point_cov.restype = i

    def call(d_P=dP, ld=L["ldp"], nn=n, h_cl=clones, n_cl=len(clones), h_jobs=jobs, n_jobs=len(jobs), h_rk=rk, h_z=z, h_zv=zv, leg=L["leg_dim"], h_out=out, h_ok=okw):
        ptr = lambda a: None if a is None else _p(a)
        h_jobs, h_rk = (None if a is None else np.ascontiguousarray(a) for a in (h_jobs, h_rk))
        return Lb.lvk_ekf_msckf_point_cov(gpu_ctx.h, ptr(d_P), ld, nn, ptr(h_cl), n_cl, ptr(h_jobs), n_jobs, ptr(h_rk), ptr(h_z), ptr(h_zv),
                                          leg, L["if_fej"], L["estimate_td"], L["sigma2"], ptr(h_out), ptr(h_ok))

    def jobs_with(k, **kw):
        j = jobs.copy()
        for key, v in kw.items():
            j[key][k] = v
        return j

    def ranks_with(pos, v):
        r = rk.copy(); r[pos] = v
        return r
    n_cl = len(clones)
    bad = [dict(d_P=None), dict(h_cl=None), dict(h_jobs=None), dict(h_rk=None), dict(h_z=None), dict(h_zv=None), dict(h_out=None), dict(h_ok=None),
           dict(n_jobs=-1), dict(ld=n - 1), dict(nn=0), dict(nn=-5), dict(h_jobs=jobs_with(2, n_obs=1)), dict(h_jobs=jobs_with(2, n_obs=65)), dict(h_jobs=jobs_with(2, n_obs=0)),
           dict(h_rk=ranks_with(4, -1)), dict(h_rk=ranks_with(4, n_cl)),            # the rank's six columns leave [0, n) on either side
           dict(h_rk=ranks_with(4, rk[3])),                                          # a rank twice in one job (observations 3..5 are job 1)
           dict(leg=23), dict(leg=0), dict(h_jobs=jobs_with(2, obs_off=-1)), dict(n_cl=-1), dict(n_cl=int(rk.max()))]      # (the largest rank is then outside the table)
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(out == 7.0) and np.all(okw == 7)                # nothing written
        assert b"lvk_ekf_msckf_point_cov" in Lb.lvk_last_error(gpu_ctx.h)
        again, ok = _run(gpu_ctx, L)
        assert np.array_equal(again.view(np.uint64), good.view(np.uint64)) and np.all(ok == 1)
    # the column boundary on its own: ONE job of two observations, ranks 0 and the last clone's; n one short of that clone's last column
    j1 = jobs[:1].copy(); j1["n_obs"] = 2; j1["obs_off"] = 0
    r1 = np.array([0, n_cl - 1], np.int32); n_fit = L["leg_dim"] + 6 * n_cl
    assert call(h_jobs=j1, n_jobs=1, h_rk=r1, nn=n_fit - 1) == 1 and np.all(out == 7.0) and np.all(okw == 7)
    assert b"does not fit" in Lb.lvk_last_error(gpu_ctx.h)
    assert call(h_jobs=j1, n_jobs=1, h_rk=r1, nn=n_fit) == 0 and okw[0] == 1 and np.all(okw[1:] == 7)      # ... and with that column it runs
    out[:] = 7.0; okw[:] = 7
    assert call(n_jobs=0) == 0 and np.all(out == 7.0)                  # LVK_OK, nothing to do
    assert call() == 0 and np.array_equal(out.reshape(-1, 3, 3).view(np.uint64), good.view(np.uint64)) and np.all(okw == 1)
