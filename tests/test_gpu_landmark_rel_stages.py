"""lvk_ekf_landmark_rel_cov (k_landmark_rel_cov, be_landmark_rel.hip) against the long-double restatement tests/landmark_rel_ref.py, inside
the componentwise bounds derived there: n = 29 with the target the anchor clone and with the target the IMU state, n = 58 with a padded
ldp and the feature in the last column, n = 60, n = 433 with 1, 65 and 300 jobs (landmark_rel_ref.stage_launches); exact symmetry;
repeatability; NaN everywhere outside a job's 19 rows and columns; every refusal."""
import numpy as np
import pytest

from tests import landmark_rel_ref as R

pytestmark = pytest.mark.gpu
LD = R.LD


def _run(ctx, L, P=None, jobs=None):
    from larvio_amd import ops
    return ops.landmark_rel_cov(ctx, R.buffer(L["P"] if P is None else P, L["n"], L["ldp"]), R.pack(L["jobs"] if jobs is None else jobs), n=L["n"])


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


@pytest.fixture(scope="module")
def launches():
    """every launch with its reference: (p_c, err_p, Sigma, err, Bnd) per job, computed once"""
    return [(L, [R.tracked(j, L["P"]) for j in L["jobs"]]) for L in R.stage_launches()]


@pytest.fixture(scope="module")
def results(gpu_ctx, launches):
    return [_run(gpu_ctx, L) for L, _ in launches]


def test_stage_entry_against_the_restatement_within_the_derived_bound(launches, results):
    worst = 0.0
    for (L, ref), (pc, S) in zip(launches, results):
        w = wp = 0.0
        for k, (pc0, err_p, S0, err, Bnd) in enumerate(ref):
            assert np.all(np.isfinite(pc[k])) and np.all(np.isfinite(S[k]))
            wp = max(wp, float(np.max(np.abs(pc[k].astype(LD) - pc0) / err_p)))
            w = max(w, float(np.max(np.abs(S[k].astype(LD) - S0) / err)))
        print("%-12s n %3d ldp %3d jobs %3d: worst |error| / bound: Sigma %.3f, p_c %.3f" % (L["name"], L["n"], L["ldp"], len(ref), w, wp))
        worst = max(worst, w, wp)
    print("worst |error| / bound %.3f" % worst)
    assert worst <= 1.0


def test_sigma_is_exactly_symmetric_and_two_calls_give_the_same_bits(gpu_ctx, launches, results):
    for (L, _), (pc, S) in zip(launches, results):
        assert np.array_equal(_bits(S), _bits(np.swapaxes(S, 1, 2)))
        pc2, S2 = _run(gpu_ctx, L)
        assert np.array_equal(_bits(pc2), _bits(pc)) and np.array_equal(_bits(S2), _bits(S))


def test_nothing_of_P_outside_the_jobs_rows_and_columns_is_read(gpu_ctx, launches, results):
    for (L, _), (pc, S) in zip(launches, results):
        for k in list(range(len(L["jobs"])))[:6]:
            j = L["jobs"][k]
            c = R.columns(j)
            keep = np.zeros((L["n"], L["n"]), bool); keep[np.ix_(c, c)] = True
            pc1, S1 = _run(gpu_ctx, L, P=np.where(keep, L["P"], np.nan), jobs=[j])
            assert np.array_equal(_bits(S1[0]), _bits(S[k])) and np.array_equal(_bits(pc1[0]), _bits(pc[k])), (L["name"], k)


def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx, launches, results):
    import ctypes as C
    from larvio_amd._lib import lib, _p
    L, _ = launches[3]; good_pc, good_S = results[3]                          # n = 60: two clones, target a clone, the IMU state, the anchor
    jobs = R.pack(L["jobs"]); n = L["n"]
    Lb = lib(); dP = gpu_ctx.to_device(R.buffer(L["P"], n, L["ldp"]))
    out = np.full((len(jobs), 12), 7.0)
    vp, i = C.c_void_p, C.c_int
    Lb.lvk_ekf_landmark_rel_cov.argtypes = [vp, vp, i, i, vp, i, vp]; Lb.lvk_ekf_landmark_rel_cov.restype = i

    def call(d_P=dP, ld=L["ldp"], nn=n, h_jobs=jobs, n_jobs=len(jobs), h_out=out, ctx=gpu_ctx.h):
        ptr = lambda a: None if a is None else _p(a)
        return Lb.lvk_ekf_landmark_rel_cov(ctx, ptr(d_P), ld, nn, ptr(h_jobs), n_jobs, ptr(h_out))

    def jobs_with(k, **kw):
        j = jobs.copy()
        for key, v in kw.items():
            j[key][k] = v
        return j

    def same_as_before():
        pc, S = _run(gpu_ctx, L)
        return np.array_equal(_bits(pc), _bits(good_pc)) and np.array_equal(_bits(S), _bits(good_S))
    bad = [dict(d_P=None), dict(h_jobs=None), dict(h_out=None), dict(n_jobs=-1), dict(ld=n - 1), dict(nn=20), dict(nn=0), dict(nn=-5)]
    for key, width in (("anchor_col", 6), ("b_theta_col", 3), ("b_p_col", 3), ("feat_col", 1)):
        bad += [dict(h_jobs=jobs_with(1, **{key: -1})), dict(h_jobs=jobs_with(1, **{key: n - width + 1})), dict(h_jobs=jobs_with(1, **{key: n})),
                dict(h_jobs=jobs_with(1, **{key: 1 << 30})), dict(h_jobs=jobs_with(len(jobs) - 1, **{key: -(1 << 30)}))]
    bad += [dict(h_jobs=jobs_with(0, inv_depth=0.0)), dict(h_jobs=jobs_with(len(jobs) - 1, inv_depth=-0.0))]
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(out == 7.0)                                     # nothing written
        assert b"lvk_ekf_landmark_rel_cov" in Lb.lvk_last_error(gpu_ctx.h)
        assert same_as_before()
    assert call(ctx=None) == 1 and np.all(out == 7.0)
    # the column boundaries on their own: each range ends at n - 1 exactly
    for key, width in (("anchor_col", 6), ("b_theta_col", 3), ("b_p_col", 3), ("feat_col", 1)):
        assert call(h_jobs=jobs_with(1, **{key: n - width}), n_jobs=2) == 0 and np.all(out[2:] == 7.0)
        out[:] = 7.0
    assert call(n_jobs=0) == 0 and np.all(out == 7.0)                  # LVK_OK, nothing to do
    assert call() == 0 and np.array_equal(_bits(out[:, :3]), _bits(good_pc)) and np.array_equal(_bits(out[:, 3:].reshape(-1, 3, 3)), _bits(good_S))
