"""lvk_ekf_pose_rel_cov (k_pose_rel_cov, be_pose_rel.hip) against the long-double restatement tests/pose_rel_ref.py, inside the
componentwise bound derived there: 1 / 2 / 61 / 300 jobs, n = 28, 46 + 12 and 433, ldp = n and padded, a on the IMU state (columns 0 and
6), b on the last six columns of n, a == b, |d| = 0, absolute jobs among relative ones (pose_rel_ref.stage_launches); absolute results
as the bits of P; exact symmetry; repeatability; NaN everywhere outside a job's rows and columns; every refusal."""
import numpy as np
import pytest

from tests import pose_rel_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _run(ctx, L, P=None, jobs=None):
    from larvio_amd import ops
    return ops.pose_rel_cov(ctx, R.buffer(L["P"] if P is None else P, L["n"], L["ldp"]), R.pack(L["jobs"] if jobs is None else jobs), n=L["n"])


@pytest.fixture(scope="module")
def launches():
    """every launch with its reference: (Sigma, bound, Bnd) per relative job (None for an absolute one), computed once"""
    return [(L, [None if j["a"] is None else R.sigma_tracked(j, L["P"]) for j in L["jobs"]]) for L in R.stage_launches()]


@pytest.fixture(scope="module")
def results(gpu_ctx, launches):
    return [_run(gpu_ctx, L) for L, _ in launches]


def test_the_launches_cover_the_job_counts_and_sizes(launches):
    assert {len(L["jobs"]) for L, _ in launches} >= {1, 2, 61, 300}
    assert {L["n"] for L, _ in launches} == {28, 58, 433} and {L["ldp"] - L["n"] for L, _ in launches} == {0, R.PAD}
    jobs = [(L, j) for L, _ in launches for j in L["jobs"]]
    assert any(j["a"] is not None and (j["a"][0], j["a"][1]) == (0, 6) for _, j in jobs)              # a on the IMU state, split columns
    assert any(j["a"] is not None and j["b"][0] == L["n"] - 6 for L, j in jobs)                      # b on the last six columns
    assert any(j["a"] is j["b"] for _, j in jobs)
    assert any(j["a"] is not None and j["a"] is not j["b"] and np.array_equal(j["a"][3], j["b"][3]) for _, j in jobs)      # |d| = 0
    assert any(len({j["a"] is None for j in L["jobs"]}) == 2 for L, _ in launches)                     # absolute among relative


def test_stage_entry_against_the_restatement_within_the_derived_bound(launches, results):
    worst = 0.0
    for (L, ref), got in zip(launches, results):
        w = 0.0
        for k, r in enumerate(ref):
            if r is None:
                continue
            S, err, Bnd = r
            assert np.all(np.isfinite(got[k]))
            w = max(w, float(np.max(np.abs(got[k].astype(LD) - S) / err)))
        print("%-11s n %3d ldp %3d jobs %3d: worst |error| / bound %.3f" % (L["name"], L["n"], L["ldp"], len(ref), w))
        worst = max(worst, w)
    print("worst |error| / bound %.3f" % worst)
    assert worst <= 1.0


def test_absolute_jobs_return_the_bits_of_P(launches, results):
    n = 0
    for (L, _), got in zip(launches, results):
        for k, j in enumerate(L["jobs"]):
            if j["a"] is None:
                c = R.columns(j)
                assert np.array_equal(got[k].view(np.uint64), np.ascontiguousarray(L["P"][np.ix_(c, c)]).view(np.uint64)), (L["name"], k)
                n += 1
    assert n >= 60


def test_sigma_is_exactly_symmetric_and_two_calls_give_the_same_bits(gpu_ctx, launches, results):
    for (L, _), got in zip(launches, results):
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(np.swapaxes(got, 1, 2)).view(np.uint64))
        assert np.array_equal(_run(gpu_ctx, L).view(np.uint64), got.view(np.uint64))


def test_nothing_of_P_outside_the_jobs_rows_and_columns_is_read(gpu_ctx, launches, results):
    for (L, _), got in zip(launches, results):
        for k in list(range(len(L["jobs"])))[:6]:
            j = L["jobs"][k]
            c = R.columns(j)
            keep = np.zeros((L["n"], L["n"]), bool); keep[np.ix_(c, c)] = True
            one = _run(gpu_ctx, L, P=np.where(keep, L["P"], np.nan), jobs=[j])
            assert np.array_equal(one[0].view(np.uint64), got[k].view(np.uint64)), (L["name"], k)


def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx, launches, results):
    import ctypes as C
    from larvio_amd._lib import lib, _p
    L, _ = launches[1]; good = results[1]                                     # n = 28, padded, absolute and relative jobs
    jobs = R.pack(L["jobs"]); n = L["n"]
    Lb = lib(); dP = gpu_ctx.to_device(R.buffer(L["P"], n, L["ldp"]))
    out = np.full((len(jobs), 36), 7.0)
    vp, i = C.c_void_p, C.c_int
    Lb.lvk_ekf_pose_rel_cov.argtypes = [vp, vp, i, i, vp, i, vp]; Lb.lvk_ekf_pose_rel_cov.restype = i

    def call(d_P=dP, ld=L["ldp"], nn=n, h_jobs=jobs, n_jobs=len(jobs), h_out=out, ctx=gpu_ctx.h):
        ptr = lambda a: None if a is None else _p(a)
        return Lb.lvk_ekf_pose_rel_cov(ctx, ptr(d_P), ld, nn, ptr(h_jobs), n_jobs, ptr(h_out))

    def jobs_with(k, **kw):
        j = jobs.copy()
        for key, v in kw.items():
            j[key][k] = v
        return j
    assert jobs["a_theta_col"][0] < 0 and jobs["a_theta_col"][1] >= 0        # job 0 absolute, job 1 relative
    bad = [dict(d_P=None), dict(h_jobs=None), dict(h_out=None), dict(n_jobs=-1), dict(ld=n - 1), dict(nn=0), dict(nn=-5)]
    for key in ("a_theta_col", "a_p_col", "b_theta_col", "b_p_col"):
        bad += [dict(h_jobs=jobs_with(1, **{key: n - 2})), dict(h_jobs=jobs_with(1, **{key: n})), dict(h_jobs=jobs_with(1, **{key: 1 << 30}))]
    bad += [dict(h_jobs=jobs_with(1, a_p_col=-1)), dict(h_jobs=jobs_with(1, b_theta_col=-1)), dict(h_jobs=jobs_with(1, b_p_col=-4)),
            dict(h_jobs=jobs_with(0, b_theta_col=n - 2)), dict(h_jobs=jobs_with(0, b_p_col=-1)), dict(h_jobs=jobs_with(len(jobs) - 1, b_p_col=n - 1))]
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(out == 7.0)                                     # nothing written
        assert b"lvk_ekf_pose_rel_cov" in Lb.lvk_last_error(gpu_ctx.h)
        assert np.array_equal(_run(gpu_ctx, L).view(np.uint64), good.view(np.uint64))
    assert call(ctx=None) == 1 and np.all(out == 7.0)
    # the column boundary on its own: b's position columns end at n - 1 exactly
    assert call(h_jobs=jobs_with(1, b_p_col=n - 3), n_jobs=2) == 0 and np.all(out[2:] == 7.0)
    out[:] = 7.0
    # an absolute job ignores its a_p_col
    assert call(h_jobs=jobs_with(0, a_p_col=1 << 30), n_jobs=1) == 0 and np.array_equal(out[0].view(np.uint64), good[0].ravel().view(np.uint64))
    out[:] = 7.0
    assert call(n_jobs=0) == 0 and np.all(out == 7.0)                  # LVK_OK, nothing to do
    assert call() == 0 and np.array_equal(out.reshape(-1, 6, 6).view(np.uint64), good.view(np.uint64))
