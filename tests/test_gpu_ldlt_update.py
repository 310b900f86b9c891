"""The pivoted LDL^T route of the measurement update (larvio_amd/csrc/be_ldlt.hip): the stage entry lvk_ekf_update_ldlt against the
long-double restatement of tests/ldlt_ref.py within its derived forward-error bound, the gate that leaves P untouched when the
Cholesky route fails, and the filter's LVK_INDEFINITE_LDLT policy.

Tie rule: on an exact tie of the remaining |diagonal| the first index wins (kernel and restatement alike).  The pivot order is
only comparable where no step is a near-tie, so every problem here is drawn (seed search on the CPU, before anything runs on the
GPU) such that the runner-up differs from the pivot by more than 1e-6 relative at EVERY step of the restatement's factorisation: no
case is left out, and the permutation must then be equal, not just close."""
import numpy as np
import pytest

from tests import ldlt_ref as R

pytestmark = pytest.mark.gpu

S2 = 0.008 ** 2
GAP = 1e-6


def _update_problem(seed, N, m):
    """the construction of tests/test_gpu_backend.py::_update_problem"""
    rng = np.random.default_rng(seed)
    Bm = rng.normal(0, 1, (N, N)); P = Bm @ Bm.T * 1e-3 + np.diag(rng.uniform(1e-8, 1e-2, N))
    H = rng.normal(0, 1, (m, N)) * (rng.uniform(0, 1, (m, N)) < 0.2); H[:, :15] = 0
    r = rng.normal(0, 0.01, m)
    return P, H, r


def _indefinite_problem(N, m, bad):
    """... made indefinite as test_ekf_update_reports_a_non_positive_definite_innovation does: direction 30 has variance -1 and is
    seen by measurement row `bad` only.  The seed is the first from N + m on whose factorisation has no near-tie."""
    for seed in range(N + m, N + m + 200):
        P, H, r = _update_problem(seed, N, m)
        H[:, 30] = 0.0; H[bad, :] = 0.0; H[bad, 30] = 1.0
        P[30, :] = 0.0; P[:, 30] = 0.0; P[30, 30] = -1.0
        ref = R.ekf_update_ldlt(P, H, r, S2)
        if ref["gaps"].min() > GAP:
            return P, H, r, ref
    raise AssertionError("no seed without a near-tie")


def _definite_problem(N, m):
    for seed in range(N + m, N + m + 200):
        P, H, r = _update_problem(seed, N, m)
        ref = R.ekf_update_ldlt(P, H, r, S2)
        if ref["gaps"].min() > GAP:
            return P, H, r, ref
    raise AssertionError("no seed without a near-tie")


def _filter_ld(n):
    return ((n + 15) & ~15) + 8


def _check_against_bound(dx, Pn, P, H, r, ref, what):
    """-> (worst ratio of dx, of P) to the derived bound; asserts both <= 1"""
    bdx, bP = R.forward_bound(P, H, r, S2, ref)
    # The first-order analysis stands while the relative perturbation eps is small: the neglected terms multiply the bound by
    # 1 / (1 - eps), which the factor 2 in forward_bound covers for eps <= 1/2.  eps is of the size of bound / solution (largest
    # entries); the problems must keep that below 0.1, five times inside what the factor 2 allows (the largest here, the 450- and
    # 485-row definite problems, have 0.025).  This is a property of the problem and the restatement alone: nothing the kernel
    # returns enters it.
    assert float(bP.max()) < 0.1 * float(np.abs(ref["P"]).max()) and float(bdx.max()) < 0.1 * max(float(np.abs(ref["dx"]).max()), 1e-300), what
    ex = np.abs(np.asarray(dx, R.LD) - ref["dx"]); eP = np.abs(np.asarray(Pn, R.LD) - ref["P"])
    rx = float(np.max(np.where(bdx > 0, ex / np.where(bdx > 0, bdx, 1), np.where(ex > 0, np.inf, 0))))
    rP = float(np.max(np.where(bP > 0, eP / np.where(bP > 0, bP, 1), np.where(eP > 0, np.inf, 0))))
    print(f"{what}: worst |error| / bound: dx {rx:.3e}  P {rP:.3e}   (max bound / max value: dx {float(bdx.max() / max(np.abs(ref['dx']).max(), 1e-300)):.2e}, P {float(bP.max() / np.abs(ref['P']).max()):.2e})")
    assert rx <= 1.0 and rP <= 1.0, (what, rx, rP)
    return rx, rP


# the four cases of the existing non-positive-definite test; m = 1, 2; the wave edges 63 / 64 / 65; the factor kernel's panel
# edges (16 columns per panel: 15 / 16 / 17, 32 / 33) and its last-panel sizes
CASES = [(120, 40, 7), (232, 150, 149), (232, 200, 170), (232, 330, 5),
         (46, 1, 0), (46, 2, 1), (120, 63, 62), (120, 64, 0), (120, 65, 64), (60, 15, 3), (60, 16, 15), (60, 17, 16), (80, 32, 31), (80, 33, 32)]


# ... and four of the shapes again in buffers with the filter's padded leading dimension
PADDED = [(120, 40, 7), (232, 330, 5), (60, 17, 16), (46, 1, 0)]


@pytest.mark.parametrize("N,m,bad,padded", [c + (False,) for c in CASES] + [c + (True,) for c in PADDED])
def test_update_ldlt_matches_the_restatement_within_the_derived_bound(gpu_ctx, N, m, bad, padded):
    from larvio_amd import larvio as lv
    P, H, r, ref = _indefinite_problem(N, m, bad)
    assert ref["info"][0] >= 1
    ld = _filter_ld(N) if padded else None
    dx, buf, info, perm = lv.ekf_update_ldlt(gpu_ctx, P, H, r, S2, ld=ld, with_perm=True)
    Pn = buf[:, :N]
    if padded:                                               # NaN-poisoned padding comes back untouched
        assert np.array_equal(buf[:, N:].view(np.uint64), np.full((N, ld - N), np.nan).view(np.uint64))
    assert np.array_equal(perm, ref["perm"]), (perm, ref["perm"])
    assert info == ref["info"], (info, ref["info"])
    assert np.array_equal(Pn, Pn.T)
    _check_against_bound(dx, Pn, P, H, r, ref, f"indefinite N {N} m {m} bad {bad}{' padded' if padded else ''}")


def _both_routes_within_the_bound(gpu_ctx, N, m):
    from larvio_amd import larvio as lv
    P, H, r, ref = _definite_problem(N, m)
    assert ref["info"] == (0, 0)
    dx_l, P_l, info, perm = lv.ekf_update_ldlt(gpu_ctx, P, H, r, S2, with_perm=True)
    dx_c, P_c = lv.ekf_update(gpu_ctx, P, H, r, S2)
    assert info == (0, 0) and np.array_equal(perm, ref["perm"])
    assert np.array_equal(P_l, P_l.T)
    _check_against_bound(dx_l, P_l, P, H, r, ref, f"definite N {N} m {m}")
    bdx, bP = R.forward_bound(P, H, r, S2, ref)
    assert (np.abs(np.asarray(dx_l, R.LD) - dx_c) <= 2 * bdx).all() and (np.abs(np.asarray(P_l, R.LD) - P_c) <= 2 * bP).all()


@pytest.mark.parametrize("N,m", [(232, 262), (118, 40), (46, 9), (232, 530), (250, 1), (232, 160), (232, 161), (232, 192), (240, 320), (330, 321), (460, 450), (470, 485)])
def test_update_ldlt_agrees_with_the_cholesky_route_on_definite_problems(gpu_ctx, N, m):
    """the twelve shapes of test_ekf_update_matches_oracle; both routes within the bound of the restatement, hence within twice the
    bound of each other.  m = 485 and 530 need more than 64 KB of dynamic LDS in the factor kernel (its opt-in), N reaches 470."""
    _both_routes_within_the_bound(gpu_ctx, N, m)


@pytest.mark.parametrize("N,m", [(47, 33), (48, 32), (63, 64), (64, 65), (127, 96), (128, 129), (232, 159)])
def test_update_routes_agree_at_the_solver_and_panel_edges(gpu_ctx, N, m):
    """the same assertions with the right-hand side's width N + 1 on the 16-column wavefront edges (48, 49) and the 64-column workgroup
    edges (64, 65, 128, 129) of the Cholesky route's solver, and m on its 32-row panel edges and at 159 - through the real lvk_ekf_update"""
    _both_routes_within_the_bound(gpu_ctx, N, m)


@pytest.mark.parametrize("N,m,bad", [(120, 40, 7), (232, 150, 149), (232, 200, 170), (232, 330, 5)])
def test_failed_cholesky_update_leaves_P_bit_identical(gpu_ctx, N, m, bad):
    """the default route still fails with the same error and the same pivot, and now d_P (padding included) is exactly its input"""
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError, lib
    import ctypes as C
    P, H, r = _update_problem(N + m, N, m)
    H[:, 30] = 0.0; H[bad, :] = 0.0; H[bad, 30] = 1.0
    P[30, :] = 0.0; P[:, 30] = 0.0; P[30, 30] = -1.0
    ld = _filter_ld(N)
    Pb, Hb = lv._padded(P, ld), lv._padded(H, ld)
    dP, dH, dr = gpu_ctx.to_device(Pb), gpu_ctx.to_device(Hb), gpu_ctx.to_device(r)
    dx0 = np.full(N, 7.25); ddx = gpu_ctx.to_device(dx0)
    lv._L()
    rc = lib().lvk_ekf_update(gpu_ctx.h, lv._p(dP), ld, N, lv._p(dH), ld, m, lv._p(dr), C.c_double(S2), lv._p(ddx))
    assert rc == 5
    with pytest.raises(LvkError) as ei:
        gpu_ctx.check(rc)
    assert "not positive definite" in str(ei.value) and f"pivot {bad})" in str(ei.value), str(ei.value)
    assert np.array_equal(gpu_ctx.to_host(dP, np.float64, Pb.shape).view(np.uint64), Pb.view(np.uint64))
    assert np.array_equal(gpu_ctx.to_host(ddx, np.float64, (N,)), dx0)
    # the same device buffers go straight to the pivoted route
    info = np.zeros(2, np.int32)
    gpu_ctx.check(lib().lvk_ekf_update_ldlt(gpu_ctx.h, lv._p(dP), ld, N, lv._p(dH), ld, m, lv._p(dr), C.c_double(S2), lv._p(ddx), lv._p(info)))
    assert info[0] == 1 and info[1] == 0
    assert np.isfinite(gpu_ctx.to_host(dP, np.float64, Pb.shape)[:, :N]).all()


def test_update_ldlt_checks_its_arguments(gpu_ctx):
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError, lib
    import ctypes as C
    lv._L()
    P, H, r = _update_problem(3, 40, 9)
    dP, dH, dr, ddx = gpu_ctx.to_device(P), gpu_ctx.to_device(H), gpu_ctx.to_device(r), gpu_ctx.alloc(8 * 40)
    info = np.zeros(2, np.int32)
    f = lib().lvk_ekf_update_ldlt
    assert f(gpu_ctx.h, lv._p(dP), 39, 40, lv._p(dH), 40, 9, lv._p(dr), C.c_double(S2), lv._p(ddx), lv._p(info)) == 1       # ldp < n
    assert f(gpu_ctx.h, lv._p(dP), 40, 40, lv._p(dH), 40, 9, lv._p(dr), C.c_double(S2), lv._p(ddx), None) == 1             # no h_info
    assert f(gpu_ctx.h, lv._p(dP), 40, 40, None, 40, 9, lv._p(dr), C.c_double(S2), lv._p(ddx), lv._p(info)) == 1
    assert f(gpu_ctx.h, lv._p(dP), 40, 40, lv._p(dH), 40, 4000, lv._p(dr), C.c_double(S2), lv._p(ddx), lv._p(info)) == 3   # LVK_ERR_CAPACITY, nothing launched
    # m = 0: nothing to do, dx = 0, P as it was
    info[:] = 9
    assert f(gpu_ctx.h, lv._p(dP), 40, 40, None, 40, 0, None, C.c_double(S2), lv._p(ddx), lv._p(info)) == 0
    assert np.array_equal(gpu_ctx.to_host(ddx, np.float64, (40,)), np.zeros(40)) and info.tolist() == [0, 0]
    assert np.array_equal(gpu_ctx.to_host(dP, np.float64, P.shape), P)


def _static_run():
    from larvio_amd import synthetic as S
    from tests.test_gpu_backend import _messages
    msgs, imu_all, seq = _messages(0, 70)
    cfg = S.backend_config(sw_size=12, max_features_in_one_grid=0)
    return msgs, imu_all, cfg


def _feed(f, buf, ts, msg):
    b = buf[:int(np.searchsorted(buf["t"], ts + 0.05))]
    ok, rest = f.processFeatures((ts, msg), b)
    return ok, buf[len(b) - len(rest):]


def test_filter_policy_ldlt_carries_on_where_the_default_fails(gpu_ctx):
    """Two filters start at rest (static initialiser, zero-velocity updates).  After the first zero-velocity update both get the
    same covariance with the x velocity decoupled and its variance set to -1e-2 (zupt_noise_v^2 = 1e-4: the first row of the next
    zero-velocity update then has S = sigma2 (1 - 1e-2 / 1e-4) < 0; that update has no chi-square gate in front of it).
    Default policy: the next message raises and the handle stays failed.  LVK_INDEFINITE_LDLT: it returns, one fallback is counted,
    and covariance and state equal the long-double restatement applied to the H, r, P, state of that update - read through
    lvk_ekf_last_update from the failed twin, which the gate left exactly where the update started."""
    import larvio_amd
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    msgs, imu_all, cfg = _static_run()
    A = larvio_amd.LarVio(cfg, gpu_ctx); B = larvio_amd.LarVio(cfg, gpu_ctx)
    assert A.initialize() and B.initialize()
    B.set_indefinite_policy(lv.INDEFINITE_LDLT)
    bufA = imu_all.copy(); bufB = imu_all.copy()
    k = 0
    while k < len(msgs):
        ts, msg = msgs[k]; k += 1
        okA, bufA = _feed(A, bufA, ts, msg); okB, bufB = _feed(B, bufB, ts, msg)
        assert okA == okB
        if okA and A.counters()["zupt"] >= 1:
            break
    assert A.counters()["zupt"] >= 1 and k < len(msgs) - 12, "no zero-velocity update at the start of the sequence"
    P = A.cov(); assert np.array_equal(P, B.cov())
    # set_cov / get_cov round trip, and what set_cov refuses
    A.set_cov(P); assert np.array_equal(A.cov().view(np.uint64), P.view(np.uint64))
    with pytest.raises(LvkError):
        A.set_cov(P[:-1, :-1])
    P[3, :] = 0.0; P[:, 3] = 0.0; P[3, 3] = -1e-2
    A.set_cov(P); B.set_cov(P)
    assert np.array_equal(B.cov().view(np.uint64), P.view(np.uint64))
    ts, msg = msgs[k]; k += 1
    with pytest.raises(LvkError) as ei:
        _feed(A, bufA, ts, msg)
    assert "not positive definite" in str(ei.value)
    with pytest.raises(LvkError) as ei2:                   # the handle stays failed
        _feed(A, bufA, *msgs[k])
    assert "failed state" in str(ei2.value)
    assert A.indefinite_fallbacks() == 0
    cB0 = B.counters()
    okB, bufB = _feed(B, bufB, ts, msg)
    assert okB and B.indefinite_fallbacks() == 1
    cB1 = B.counters()
    assert cB1["zupt"] == cB0["zupt"] + 1
    H, r, P0, s0 = A.last_update()
    assert H.shape[0] == 9
    ref = R.ekf_update_ldlt(P0, H, r, float(cfg["noise_feature"]) ** 2)
    assert ref["info"][0] >= 1
    bdx, bP = R.forward_bound(P0, H, r, float(cfg["noise_feature"]) ** 2, ref)
    Pn = B.cov(); sB = B.state()
    # Later stages of the same message (lost features, pruning) did not update again (counters) - they may have dropped clone
    # columns, which moves no value of the IMU block; with the dimension unchanged the whole matrix is compared.
    assert cB1["hybrid"] == cB0["hybrid"] and cB1["msckf"] == cB0["msckf"], (cB0, cB1)
    nc = P0.shape[0] if Pn.shape == P0.shape else 22
    eP = np.abs(np.asarray(Pn[:nc, :nc], R.LD) - ref["P"][:nc, :nc])
    print("filter fallback: compared", nc, "of", P0.shape[0], "columns; worst |error| / bound", float(np.max(np.where(bP[:nc, :nc] > 0, eP / np.where(bP[:nc, :nc] > 0, bP[:nc, :nc], 1), 0))))
    assert (eP <= bP[:nc, :nc]).all()
    assert np.array_equal(Pn, Pn.T)
    # state: v, p, bg, ba are corrected additively by dx[3:15] (the quaternion by a small-angle product, not restated here)
    pre = np.concatenate([s0[5:8], s0[8:11], s0[11:14], s0[14:17]])
    post = np.concatenate([np.asarray(sB[kk], np.float64).ravel() for kk in ("v", "p", "bg", "ba")])
    exp = np.asarray(pre, R.LD) + ref["dx"][3:15]
    assert (np.abs(np.asarray(post, R.LD) - exp) <= bdx[3:15] + 2 * R.U * np.abs(exp)).all(), (post, np.asarray(exp, np.float64))
    n_more = 0
    while k < len(msgs) and n_more < 12:
        ts, msg = msgs[k]; k += 1
        okB, bufB = _feed(B, bufB, ts, msg); n_more += 1
    assert n_more >= 10
    assert np.isfinite(B.cov()).all() and np.isfinite(np.asarray(B.state()["p"])).all()
    print("fallbacks after", n_more, "more messages:", B.indefinite_fallbacks(), "min diag P", float(np.diag(B.cov()).min()))
    A.close(); B.close()


def test_filter_policy_ldlt_through_the_deferred_path_and_refusals(gpu_ctx):
    """the same through lvk_ekf_process_async / lvk_ekf_wait; set_cov is refused between the queueing of an update and the first call
    that waits for it (whether the worker has finished or not: nothing here depends on timing)"""
    import larvio_amd
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    msgs, imu_all, cfg = _static_run()
    B = larvio_amd.LarVio(cfg, gpu_ctx)
    assert B.initialize()
    with pytest.raises(LvkError):
        B.set_indefinite_policy(2)
    B.set_indefinite_policy(lv.INDEFINITE_LDLT)
    buf = imu_all.copy()
    k = 0
    while k < len(msgs):
        ts, msg = msgs[k]; k += 1
        ok, buf = _feed(B, buf, ts, msg)
        if ok and B.counters()["zupt"] >= 1:
            break
    P = B.cov(); P[3, :] = 0.0; P[:, 3] = 0.0; P[3, 3] = -1e-2
    B.set_cov(P)
    ts, msg = msgs[k]; k += 1
    b = buf[:int(np.searchsorted(buf["t"], ts + 0.05))]
    will, rest = B.processFeaturesAsync((ts, msg), b)
    assert will
    with pytest.raises(LvkError) as ei:                    # queued and not yet waited for
        B.set_cov(P)
    assert "in flight" in str(ei.value)
    assert B.wait()
    assert B.indefinite_fallbacks() == 1
    assert np.isfinite(B.cov()).all()
    B.close()


def test_sharded_update_refuses_the_policy_both_ways(gpu_ctx):
    """LVK_ERR_UNSUPPORTED from lvk_ekf_set_indefinite_policy when a transport is set, and from lvk_ekf_set_shard when the policy is"""
    import ctypes as C
    import larvio_amd
    from larvio_amd import larvio as lv
    from larvio_amd import synthetic as S
    from larvio_amd._lib import LvkError
    cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda *a: 0)      # never called here
    fn = C.cast(cb, C.c_void_p)
    cfg = S.backend_config(sw_size=12, max_features_in_one_grid=0)
    A = larvio_amd.LarVio(cfg, gpu_ctx); assert A.initialize()
    A.set_shard(0, 1, fn, None, keepalive=cb)
    with pytest.raises(LvkError) as ei:
        A.set_indefinite_policy(lv.INDEFINITE_LDLT)
    assert "status 4" in str(ei.value) and "pivoted fallback" in str(ei.value), str(ei.value)
    A.set_indefinite_policy(lv.INDEFINITE_FAIL)            # the default is always accepted
    A.close()
    B = larvio_amd.LarVio(cfg, gpu_ctx); assert B.initialize()
    B.set_indefinite_policy(lv.INDEFINITE_LDLT)
    with pytest.raises(LvkError) as ei:
        B.set_shard(0, 1, fn, None, keepalive=cb)
    assert "pivoted fallback" in str(ei.value), str(ei.value)
    B.close()
