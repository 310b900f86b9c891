"""lvk_ekf_set_msckf_points / lvk_ekf_take_msckf_points on simulated messages (tests/feature_sim.py, sw_size 10, 41 messages): the
export is a pure observer (state, covariance and counters keep their bits), blocking and deferred runs give the same list, every record
is a usable covariance, and the points sit on the simulation's true landmarks as their covariance says.

Two configurations.  `sim` keeps max_track_len 6: features enter the state, both routes of remove_lost_features run, and a track
longer than 6 messages is consumed in pieces - each piece is a record under the track's id.  `sim_long` sets max_track_len above the
window, so a feature is consumed once, when it is lost: there the ids are distinct."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
CHI2_3_999 = 16.27            # the 99.9 % quantile of chi-square with 3 degrees of freedom


def _drive(ctx, sim, on, deferred=False):
    """-> (snapshots after every message, all points, the filter's features at the end)"""
    import larvio_amd
    gpu = larvio_amd.LarVio(sim["cfg"], ctx); assert gpu.initialize()
    if on is not None:
        gpu.set_msckf_points(on)
    gpu.set_state(*sim["init"])
    imu = sim["imu"]; lo = 0; snaps = []; pts = []; in_state = set()
    for ts, m in sim["msgs"]:
        b = imu[lo:int(np.searchsorted(imu["t"], ts + 0.05, side="left"))]
        _, rest = (gpu.processFeaturesAsync if deferred else gpu.processFeatures)((ts, m), b)
        lo += len(b) - len(rest)
        s = gpu.state(); c = gpu.counters()
        snaps.append(dict(state=np.concatenate([[s["t"]], s["q"], s["v"], s["p"], s["bg"], s["ba"], s["R_b2c"].ravel(), s["t_c_b"], [s["td"]]]), P=gpu.cov(),
                          counters=np.array([c[k] for k in sorted(c)])))
        got = gpu.take_msckf_points()
        in_state |= set(int(i) for i in gpu.features()[0]) & set(int(i) for i in got[0])
        pts.append(got)
    assert len(gpu.take_msckf_points()[0]) == 0                            # drained
    gpu.close()
    return snaps, tuple(np.concatenate([p[k] for p in pts]) for k in range(4)), in_state, [len(p[0]) for p in pts]


def _sim(**over):
    from tests import feature_sim as F
    return F.simulate(4, t1=6.0, sw_size=10, fresh_ids=True, **over)


@pytest.fixture(scope="module")
def sim():
    return _sim()


@pytest.fixture(scope="module")
def run_on(gpu_ctx, sim):
    return _drive(gpu_ctx, sim, True)


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
    assert len(run_off[1][0]) == 0
    assert len(run_on[1][0]) > 100 and sum(1 for k in run_on[3] if k) >= 10      # ... and on, most updates export


def test_blocking_and_deferred_runs_give_the_same_points(gpu_ctx, sim, run_on):
    snaps, pts, _, per = _drive(gpu_ctx, sim, True, deferred=True)
    assert per == run_on[3]
    for a, b in zip(pts, run_on[1]):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.array_equal(snaps[-1]["P"].view(np.uint64), run_on[0][-1]["P"].view(np.uint64))


def test_a_transport_and_the_switch_refuse_each_other(gpu_ctx, sim):
    import ctypes as C
    import larvio_amd
    from larvio_amd._lib import LvkError
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 0)      # never called here
    fn = C.cast(cb, C.c_void_p)
    A = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert A.initialize()
    A.set_shard(0, 1, fn, None, keepalive=cb)
    with pytest.raises(LvkError) as ei:
        A.set_msckf_points(True)
    assert "status 4" in str(ei.value) and "lvk_ekf_set_msckf_points" in str(ei.value), str(ei.value)
    A.set_msckf_points(False)                                            # off is always accepted
    A.close()
    B = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert B.initialize()
    B.set_msckf_points(True)
    with pytest.raises(LvkError) as ei:
        B.set_shard(0, 1, fn, None, keepalive=cb)
    assert "status 4" in str(ei.value) and "MSCKF points" in str(ei.value), str(ei.value)
    B.close()


def test_every_record_is_a_usable_covariance(sim, run_on):
    ids, pos, cov, n_obs = run_on[1]
    assert np.isfinite(pos).all() and np.isfinite(cov).all()
    assert np.array_equal(cov, np.swapaxes(cov, 1, 2))
    for S in cov:
        np.linalg.cholesky(S)                                            # raises unless positive definite
    assert n_obs.min() >= sim["cfg"]["least_observation_number"] and n_obs.max() <= sim["cfg"]["sw_size"] + 2
    assert not run_on[2]                                                 # none of them was an in-state feature when it was handed out


def _d2(sim, pts):
    ids, pos, cov, _ = pts
    e = pos - sim["landmarks"][ids]
    return np.einsum("ni,nij,nj->n", e, np.linalg.inv(cov), e), e


def test_points_lie_on_the_true_landmarks_as_their_covariance_says(sim, run_on):
    d2, e = _d2(sim, run_on[1])
    q = np.quantile(d2, [0.1, 0.25, 0.5, 0.75, 0.9, 0.99])
    print("%d points, |e| median %.3g m; d2 = e^T Sigma^-1 e: 10/25/50/75/90/99 %% = %s, share below %.2f: %.3f" % (len(d2), np.median(np.linalg.norm(e, axis=1)),
                                                                                                                   np.array2string(q, precision=3), CHI2_3_999, np.mean(d2 < CHI2_3_999)))
    assert np.median(d2) < CHI2_3_999


def test_ids_are_distinct_when_tracks_are_consumed_once(gpu_ctx):
    sim_long = _sim(max_track_len=14)
    _, pts, in_state, _ = _drive(gpu_ctx, sim_long, True)
    ids = pts[0]
    assert len(ids) >= 10 and len(np.unique(ids)) == len(ids) and not in_state      # (few features are lost in 4 s: a few dozen points)
    assert pts[3].min() >= sim_long["cfg"]["least_observation_number"]
    d2, _ = _d2(sim_long, pts)
    print("max_track_len 14: %d points, median d2 %.3f" % (len(ids), np.median(d2)))
    assert np.median(d2) < CHI2_3_999


def test_noise_free_points_are_inside_one_sigma(gpu_ctx):
    sim0 = _sim(sigma=0.0, imu_noise=0.0, perturb=False)
    _, pts, _, _ = _drive(gpu_ctx, sim0, True)
    d2, e = _d2(sim0, pts)
    lam = np.array([np.linalg.eigvalsh(S)[-1] for S in pts[2]])
    r = np.linalg.norm(e, axis=1) / np.sqrt(lam)
    print("noise-free: %d points, largest |e| / sqrt(lambda_max) %.3g, largest |e| %.3g m" % (len(r), r.max(), np.linalg.norm(e, axis=1).max()))
    assert len(r) > 100 and np.all(r < 1.0)
