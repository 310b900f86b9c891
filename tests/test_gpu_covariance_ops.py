"""Stage tests of the structural covariance kernels (be_linalg.hip: k_cov_propagate_augment, k_cov_gather, k_cov_reanchor,
k_cov_append_rows / k_cov_append_corner) through their C entries lvk_ekf_cov_*.

Every result is held to a plain extended-precision restatement of the reference's formula (larvio.cpp:553-571, 752-798,
1821-1854, 3125-3293), not of the kernel's decomposition, entry by entry:
  - computed entries within the componentwise forward-error bound 4 k u (|A| |B|) (k = length of the sum, u = 2^-53; a product of
    three factors: 4 (k1 + k2) u (|A| |B| |C|)) - every legitimate summation order meets it, a wrong index or a dropped term
    misses it by orders of magnitude;
  - entries that are pure copies bit-identical to their source;
  - the result exactly symmetric;
  - the buffers poisoned with NaN around the matrix (padding between n and ld, two rows past the end, the rows and columns an
    operation is to fill): every in-range entry finite, every byte the operation must not write unchanged.
P is a random SPD matrix whose variances span ten decades, so that an error in a small block cannot hide behind a large one.
The leading dimensions are the filter's (backend.hip: ((nmax + 15) & ~15) + 8), never equal to n."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
LDE = np.longdouble
SEL = (0, 1, 2, 6, 7, 8)                     # the rows a new clone copies (theta, p)


def _ld(n):
    return ((n + 15) & ~15) + 8


def _spd(rng, n, decades=10.0):
    """SPD, exactly symmetric, standard deviations spread over decades / 2 orders of magnitude (variances over `decades`)"""
    B = rng.normal(0, 1, (n, 24))
    C = B @ B.T + np.diag(rng.uniform(4.0, 40.0, n))
    d = 1.0 / np.sqrt(np.diag(C))
    s = 10.0 ** rng.uniform(-1.0 - decades / 2, -1.0, n)
    P = C * (d * s)[:, None] * (d * s)[None, :]
    return (P + P.T) / 2.0


def _poisoned(X, ld, rows):
    buf = np.full((rows, ld), np.nan)
    buf[:X.shape[0], :X.shape[1]] = X
    return buf


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_frame(out, before, n, must_keep=None):
    """out: buffer after the call, before: the same buffer before it.  [:n, :n] finite and exactly symmetric; every entry outside
    it (padding, rows past n) bit-unchanged; so is every entry of [:n, :n] where must_keep is True."""
    A = out[:n, :n]
    assert np.isfinite(A).all(), f"{int((~np.isfinite(A)).sum())} in-range entries not written (or computed from padding)"
    assert np.array_equal(A, A.T), "result not exactly symmetric"
    outside = np.ones(out.shape, bool); outside[:n, :n] = False
    if must_keep is not None:
        outside[:n, :n] = must_keep
    changed = _bits(out)[outside] != _bits(before)[outside]
    assert not changed.any(), f"{int(changed.sum())} entries written that the operation must not touch, first at {np.argwhere(outside)[np.argmax(changed)]}"


def _check_bound(out, ref, tol, what):
    err = np.abs(out.astype(LDE) - ref)
    bad = err > tol
    if bad.any():
        k = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(tol, 1e-300), 0)), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} entries outside the forward-error bound; worst at {k}: |err| {float(err[k]):.3e}, bound {float(tol[k]):.3e}, "
                             f"value {float(ref[k]):.3e}")


# ----------------------------------------------------------------------------------------------- propagate + augment
def _phi_q(rng, L, D):
    """a transition with the composed transition's structure (L = 22: rows 9.. identity, Q zero outside 15 x 15) and SPD noise of
    the size of the block's variances (D: the block's standard deviations)"""
    Phi = np.eye(L)
    rows = 9 if L == 22 else L
    Phi[:rows] += rng.normal(0, 0.3, (rows, L)) * (rng.uniform(0, 1, (rows, L)) < 0.6)
    m = 15 if L == 22 else L
    G = rng.normal(0, 1, (m, m)); Qm = G @ G.T / m * 0.1
    Qm = Qm * D[:m, None] * D[None, :m]
    Q = np.zeros((L, L)); Q[:m, :m] = (Qm + Qm.T) / 2.0
    return Phi, Q


def _propagate_augment_ref(P, pose_rows, Phi, Q):
    """processModel's covariance (larvio.cpp:553-571) then stateAugmentation's J P J^T (:752-798), in long double; returns the
    augmented reference, the componentwise bound and the map of output rows to source rows"""
    L = Phi.shape[0]; n = P.shape[0]
    Pl, F, Ql = P.astype(LDE), Phi.astype(LDE), Q.astype(LDE)
    Pp = Pl.copy()
    Pp[:L, :L] = F @ Pl[:L, :L] @ F.T + Ql
    Pp[:L, L:] = F @ Pl[:L, L:]
    Pp[L:, :L] = Pp[:L, L:].T
    Pp = (Pp + Pp.T) / 2
    bnd = np.zeros((n, n))
    aF, aP = np.abs(Phi), np.abs(P)
    bnd[:L, :L] = 4 * (2 * L + 2) * U * (aF @ aP[:L, :L] @ aF.T + np.abs(Q))
    bnd[:L, L:] = 4 * L * U * (aF @ aP[:L, L:])
    bnd[L:, :L] = bnd[:L, L:].T
    src = np.r_[np.arange(pose_rows), SEL, np.arange(pose_rows, n)]
    ix = np.ix_(src, src)
    return Pp[ix], bnd[ix], src


def _propagate_case(ctx, L, n_c, n_feat, seed, ldin=None, ldout=None):
    from larvio_amd import larvio as lv
    rng = np.random.default_rng(seed)
    n_in = L + n_c; n_out = n_in + 6; pose_rows = L + n_c - n_feat
    P = _spd(rng, n_in)
    Phi, Q = _phi_q(rng, L, np.sqrt(np.diag(P)))
    ldin = ldin or _ld(n_in); ldout = ldout or _ld(n_out) + 32
    Pin = _poisoned(P, ldin, n_in + 2)
    Pout0 = np.full((n_out + 2, ldout), np.nan)
    out = lv.cov_propagate_augment(ctx, Pin, Pout0, n_out, pose_rows, Phi, Q)
    _check_frame(out, Pout0, n_out)
    ref, bnd, src = _propagate_augment_ref(P, pose_rows, Phi, Q)
    A = out[:n_out, :n_out]
    copy = (src >= L)[:, None] & (src >= L)[None, :]
    assert np.array_equal(_bits(A)[copy], _bits(P[np.ix_(src, src)])[copy]), "copied entries (both sources outside the IMU block) not bit-identical"
    _check_bound(A, ref, bnd, f"propagate+augment L={L} n_c={n_c} features={n_feat}")
    return out


def _n_c_cases():
    for L in (22, 46):
        for n_c in (0, 1, 5, 7, 8, 9, 63, 64, 65, 6 * 30, 6 * 62):
            yield L, n_c, 0
            if n_c:
                yield L, n_c, max(1, n_c // 3)


@pytest.mark.parametrize("L,n_c,n_feat", list(_n_c_cases()))
def test_propagate_augment(gpu_ctx, L, n_c, n_feat):
    """Phi P_II Phi^T + Q, Phi P_IC, plain copies, the new clone's rows at pose_rows; clones only (n_feat 0: pose_rows = n_out - 6)
    and clones followed by in-state features; n_c = n_out - L - 6 columns outside the IMU block, around the 8 strips' edges"""
    if n_feat:      # ldin > ldout as well as ldin < ldout
        _propagate_case(gpu_ctx, L, n_c, n_feat, 100 * L + n_c + 7, ldin=_ld(L + n_c) + 64, ldout=_ld(L + n_c + 6))
    else:
        _propagate_case(gpu_ctx, L, n_c, n_feat, 100 * L + n_c)


def _propagate_lds_bytes(L, n_out):
    """the launcher's LDS size (lvk_cov_propagate_augment): max(strip, IMU block)"""
    n_c = n_out - L - 6; cc = (n_c + 7) // 8
    return 8 * max(L * L + 2 * L * max(cc, 1), 5 * L * L)


@pytest.mark.parametrize("L", [22, 46])
def test_propagate_augment_at_the_lds_capacity(gpu_ctx, L):
    """the largest n_out whose strip fits 160 KB (LDS opt-in path) computes; the next one is LVK_ERR_CAPACITY, not a failed launch,
    and the context goes on working"""
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    n_out = L + 6
    while _propagate_lds_bytes(L, n_out + 1) <= 160 * 1024:
        n_out += 1
    assert _propagate_lds_bytes(L, n_out) > 64 * 1024
    n_c = n_out - L - 6
    _propagate_case(gpu_ctx, L, n_c, n_c // 4, 5 + L)
    rng = np.random.default_rng(L)
    P = _spd(rng, n_out + 1 - 6); Phi, Q = _phi_q(rng, L, np.sqrt(np.diag(P)))
    Pout0 = np.full((n_out + 1, _ld(n_out + 1)), np.nan)
    with pytest.raises(LvkError, match="lvk status 3"):
        lv.cov_propagate_augment(gpu_ctx, _poisoned(P, _ld(n_out - 5), n_out - 5), Pout0, n_out + 1, L + 6, Phi, Q)
    _propagate_case(gpu_ctx, L, 30, 6, 11)


@pytest.mark.parametrize("bad", ["phi_row_9", "phi_row_21", "q_outside_15"])
def test_propagate_augment_refuses_what_the_l22_kernel_cannot_hold(gpu_ctx, bad):
    """the L = 22 kernel receives rows 0-8 of Phi and Q's leading 15 x 15 only: anything else is refused, not silently dropped"""
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    rng = np.random.default_rng(3)
    n_in = 22 + 30; P = _spd(rng, n_in); Phi, Q = _phi_q(rng, 22, np.sqrt(np.diag(P)))
    if bad == "phi_row_9":
        Phi[9, 3] = 1e-3
    elif bad == "phi_row_21":
        Phi[21, 21] = 1.0 + 2.0 ** -40
    else:
        Q[16, 2] = Q[2, 16] = 1e-9
    Pout0 = np.full((n_in + 6, _ld(n_in + 6)), np.nan)
    with pytest.raises(LvkError, match="lvk status 1"):
        lv.cov_propagate_augment(gpu_ctx, _poisoned(P, _ld(n_in), n_in), Pout0, n_in + 6, n_in, Phi, Q)
    _propagate_case(gpu_ctx, 22, 12, 0, 4)


# ----------------------------------------------------------------------------------------------- gather
def _gather_maps(n):
    """output dimension n: the augmentation map and the deletions backend.hip builds (clone blocks, lost in-state features)"""
    L = 22
    n_cl = max(3, min(30, (n - L - 8) // 6))
    aug_in = n - 6; pr = L + 6 * min(n_cl, (aug_in - L) // 6)
    yield "augment", aug_in, np.r_[np.arange(pr), SEL, np.arange(pr, aug_in)]
    for name, drop_clones in (("one_clone", [n_cl // 2]), ("two_clones", [1, n_cl - 1]), ("oldest_and_middle", [0, n_cl // 2])):
        n_in = n + 6 * len(drop_clones)
        drop = np.zeros(n_in, bool)
        for c in drop_clones:
            drop[L + 6 * c: L + 6 * c + 6] = True
        yield name, n_in, np.flatnonzero(~drop)
    n_in = n + 3                                                   # rmLostFeaturesCov: three in-state features, the last one included
    drop = np.zeros(n_in, bool); drop[[n_in - 1, n_in - 3, n_in - 6]] = True
    yield "lost_features", n_in, np.flatnonzero(~drop)


@pytest.mark.parametrize("n", [28, 127, 128, 129, 600])
def test_gather(gpu_ctx, n):
    """Pout = Pin[idx, idx]: every entry a bit-exact copy, nothing written outside n x n"""
    from larvio_amd import larvio as lv
    for name, n_in, idx in _gather_maps(n):
        assert len(idx) == n
        rng = np.random.default_rng(n + n_in)
        P = _spd(rng, n_in)
        Pout0 = np.full((n + 2, _ld(n) + 16), np.nan)
        out = lv.cov_gather(gpu_ctx, _poisoned(P, _ld(n_in), n_in + 2), Pout0, idx)
        _check_frame(out, Pout0, n)
        assert np.array_equal(_bits(out[:n, :n]), _bits(P[np.ix_(idx, idx)])), name


# ----------------------------------------------------------------------------------------------- re-anchor
def _reanchor_check(ctx, P, ld, J, fc):
    from larvio_amd import larvio as lv
    n = P.shape[0]
    buf = _poisoned(P, ld, n + 2)
    out = lv.cov_reanchor(ctx, buf, n, J, fc)
    keep = np.ones((n, n), bool); keep[fc, :] = False; keep[:, fc] = False
    _check_frame(out, buf, n, must_keep=keep)
    nz = np.flatnonzero(J); k = len(nz)
    Jl = J.astype(LDE); JP = Jl @ P.astype(LDE)
    ref = JP.copy(); ref[fc] = JP @ Jl                               # updateFeatureCov_1didp: row fc <- J P, (fc, fc) <- J P J^T
    aJP = np.abs(J) @ np.abs(P)
    tol = 4 * k * U * aJP; tol[fc] = 4 * 2 * k * U * (aJP @ np.abs(J))
    _check_bound(out[fc, :n], ref, tol, f"re-anchor n={n} fc={fc} nnz={k}")


def _layout(n):
    """clones and in-state features of an n-dimensional state (L = 22): at least two clones, at least one feature"""
    n_cl = max(2, min(30, (n - 23) // 6))
    return n_cl, 22 + 6 * n_cl


@pytest.mark.parametrize("n", [60, 255, 256, 257, 700, 1300])
@pytest.mark.parametrize("where", ["first_feature", "last", "column_0"])
def test_reanchor_product_pattern(gpu_ctx, n, where):
    """J with the product's 19 non-zeros: the feature itself, the old and the new anchor clone (6 each), the extrinsics (15-20).
    In the filter fc is an in-state feature, so its first possible column is the first feature's (22 + 6 clones) and its last n - 1;
    column 0 is not a feature's but the kernel takes any fc, and fc = 0 puts the row it rewrites at the start of the first pass."""
    rng = np.random.default_rng(n * 3 + len(where))
    n_cl, f0 = _layout(n)
    fc = {"first_feature": f0, "last": n - 1, "column_0": 0}[where]
    J = np.zeros(n)
    J[fc] = rng.uniform(0.5, 2.0)
    for c in (n_cl - 1, rng.integers(0, n_cl - 1)):
        J[22 + 6 * c: 22 + 6 * c + 6] = rng.normal(0, 1, 6) * 10.0 ** rng.uniform(-3, 2, 6)
    J[15:21] = rng.normal(0, 1, 6)
    assert np.count_nonzero(J) == 19
    _reanchor_check(gpu_ctx, _spd(rng, n), _ld(n), J, fc)


@pytest.mark.parametrize("n,count", [(257, 40), (700, 64), (1300, 64), (300, 64), (1300, 33)])
def test_reanchor_nonzeros_across_wave_and_pass_edges(gpu_ctx, n, count):
    """non-zeros on both sides of every 64-lane wave and 256-column pass boundary, up to the 64 the kernel holds (exactly 64: all
    of them must count)"""
    rng = np.random.default_rng(n + count)
    edges = [e + d for e in range(64, n, 64) for d in (-1, 0)][:count]
    rest = np.setdiff1d(np.arange(n), edges)
    pos = np.sort(np.r_[edges, rng.choice(rest, count - len(edges), replace=False)])
    fc = int(pos[len(pos) // 2])
    J = np.zeros(n); J[pos] = rng.normal(0, 1, len(pos)) * 10.0 ** rng.uniform(-2, 2, len(pos))
    assert np.count_nonzero(J) == count
    _reanchor_check(gpu_ctx, _spd(rng, n), _ld(n) + 8, J, fc)


def test_reanchor_refuses_more_than_64_nonzeros(gpu_ctx):
    """k_cov_reanchor keeps 64 non-zeros and would drop the rest silently: the entry refuses 65 and leaves P as it was"""
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    n = 400; rng = np.random.default_rng(65)
    J = np.zeros(n); J[rng.choice(n, 65, replace=False)] = 1.0
    fc = int(np.flatnonzero(J)[0])
    P = _spd(rng, n)
    with pytest.raises(LvkError, match="lvk status 1"):
        lv.cov_reanchor(gpu_ctx, _poisoned(P, _ld(n), n), n, J, fc)
    J[np.flatnonzero(J)[-1]] = 0.0
    _reanchor_check(gpu_ctx, P, _ld(n), J, fc)


@pytest.mark.parametrize("op", ["reanchor", "append"])
def test_row_kernels_report_their_lds_capacity(gpu_ctx, op):
    """k_cov_reanchor / k_cov_append_rows hold n + 256 doubles in LDS without opting in above 64 KB: one past that is
    LVK_ERR_CAPACITY, not a failed launch; the largest n that fits still computes.  One zeroed device buffer serves both n; only the
    rows the operation reads or writes cross to the host."""
    import ctypes as C
    from larvio_amd import larvio as lv
    from larvio_amd._lib import lib
    n_fit = 64 * 1024 // 8 - 256
    ld = _ld(n_fit + 2)
    dP = gpu_ctx.alloc(8 * ld * (n_fit + 2))
    L = lv._L()

    def put_row(r, vals):
        row = np.ascontiguousarray(vals, np.float64)
        gpu_ctx.check(lib().lvk_memcpy_h2d(gpu_ctx.h, C.c_void_p(dP.ptr + 8 * r * ld), row.ctypes.data_as(C.c_void_p), row.nbytes))

    def row(r, n):
        return gpu_ctx.to_host(dP.ptr + 8 * r * ld, np.float64, (n,))

    for n, ok in ((n_fit + 1, False), (n_fit, True)):
        gpu_ctx.check(lib().lvk_memset(gpu_ctx.h, C.c_void_p(dP.ptr), 0, dP.nbytes))
        rows = {0: (0, 1e-2), 5: (5, 1e-2), n - 1: (n - 1, 1e-2)}       # diagonal entries, and P[0, n-1] = P[n-1, 0] = 1e-3
        for r, (c, v) in rows.items():
            x = np.zeros(n); x[c] = v
            if r in (0, n - 1):
                x[n - 1 - r] = 1e-3
            put_row(r, x)
        if op == "reanchor":
            J = np.zeros(n); J[[0, 5, n - 1]] = (0.5, 2.0, 1.5)
            st = L.lvk_ekf_cov_reanchor(gpu_ctx.h, C.c_void_p(dP.ptr), ld, n, J.ctypes.data_as(C.c_void_p), n - 1)
            if not ok:
                assert st == 3, st
                continue
            gpu_ctx.check(st)
            fc = row(n - 1, n)
            # J P: column 0 <- 0.5e-2 + 1.5e-3, column 5 <- 2e-2, column n-1 (J P J^T) <- 0.5 * (0.5e-3 + 1.5e-2) + 1.5 * (0.5e-3 + 1.5e-2) ...
            assert fc[0] == 0.5 * 1e-2 + 1.5 * 1e-3 and fc[5] == 2.0 * 1e-2 and not fc[1:5].any() and not fc[6:n - 1].any()
            jp_fc = 0.5 * 1e-3 + 1.5 * 1e-2
            assert abs(fc[n - 1] - (fc[0] * 0.5 + fc[5] * 2.0 + jp_fc * 1.5)) <= 1e-16
            for r, want in ((0, fc[0]), (5, fc[5]), (1, 0.0), (n - 2, 0.0)):          # column n-1 mirrors the row
                assert row(r, n)[n - 1] == want, r
            assert row(5, n)[5] == 1e-2 and row(0, n)[0] == 1e-2
        else:
            H1 = np.zeros(n); H1[[0, n - 1]] = (1.0, -2.0)
            dH1, dr1, ddx, dxn = gpu_ctx.to_device(H1), gpu_ctx.to_device(np.array([0.1])), gpu_ctx.to_device(np.zeros(n)), gpu_ctx.alloc(8)
            H2 = np.array([0.5])
            st = L.lvk_ekf_cov_append_features(gpu_ctx.h, C.c_void_p(dP.ptr), ld, n, 1, C.c_void_p(dH1.ptr), n, H2.ctypes.data_as(C.c_void_p),
                                               C.c_void_p(dr1.ptr), C.c_void_p(ddx.ptr), 1e-4, C.c_void_p(dxn.ptr))
            if not ok:
                assert st == 3, st
                continue
            gpu_ctx.check(st)
            new = row(n, n + 1)
            # HH = H1 / 0.5 = (2, ..., -4):  -HH P = (-(2e-2 - 4e-3), ..., -(2e-3 - 4e-2)), corner HH P HH^T + 1e-4 / 0.25
            assert new[0] == -(2.0 * 1e-2 + -4.0 * 1e-3) and new[n - 1] == -(2.0 * 1e-3 + -4.0 * 1e-2) and not new[1:n - 1].any()
            assert abs(new[n] - (-(new[0] * 2.0 + new[n - 1] * -4.0) + 1e-4 / 0.25)) <= 1e-16
            assert row(0, n + 1)[n] == new[0] and row(n - 1, n + 1)[n] == new[n - 1] and row(7, n + 1)[n] == 0.0
            assert gpu_ctx.to_host(dxn, np.float64, (1,))[0] == 0.1 / 0.5


# ----------------------------------------------------------------------------------------------- append features
@pytest.mark.parametrize("n", [40, 63, 64, 65, 232, 700])
@pytest.mark.parametrize("nn", [1, 2, 3, 7, 16, 40])
def test_append_features(gpu_ctx, n, nn):
    """delayed initialisation (larvio.cpp:1821-1854): P_new,old = -HH P, P_new,new = HH P HH^T + sigma2 (H2^T H2)^-1, dx_new =
    -HH dx + H2^-1 r1 with HH = H2^-1 H1; H2 of both signs from 1e-3 to 1e3; the old block bit-unchanged"""
    from larvio_amd import larvio as lv
    rng = np.random.default_rng(n * 100 + nn)
    P = _spd(rng, n)
    ld = _ld(n + nn + 8)
    H1 = rng.normal(0, 1, (nn, n)) * (rng.uniform(0, 1, (nn, n)) < 0.4) * 10.0 ** rng.uniform(-2, 2, (nn, n))
    H1[:, n - 1] = rng.normal(0, 1, nn)                                # the last column is always used
    H2 = rng.choice([-1.0, 1.0], nn) * 10.0 ** rng.uniform(-3, 3, nn)
    r1 = rng.normal(0, 1e-2, nn); dx = rng.normal(0, 1, n) * np.sqrt(np.diag(P)); sigma2 = 0.008 ** 2
    buf = _poisoned(P, ld, n + nn + 2)
    out, dx_new = lv.cov_append_features(gpu_ctx, buf, n, _poisoned(H1, _ld(n), nn + 1), H2, r1, dx, sigma2)
    N = n + nn
    keep = np.zeros((N, N), bool); keep[:n, :n] = True
    _check_frame(out, buf, N, must_keep=keep)
    HH = H1.astype(LDE) / H2.astype(LDE)[:, None]
    nHHP = -HH @ P.astype(LDE)
    P22 = -nHHP @ HH.T + np.diag(LDE(sigma2) / H2.astype(LDE) ** 2)
    aHH = np.abs(H1 / H2[:, None]); aHHP = aHH @ np.abs(P)
    _check_bound(out[n:N, :n], nHHP, 4 * (n + 2) * U * aHHP, f"P_new,old n={n} nn={nn}")
    _check_bound(out[n:N, n:N], P22, 4 * (2 * n + 6) * U * (aHHP @ aHH.T + np.diag(sigma2 / H2 ** 2)), f"P_new,new n={n} nn={nn}")
    dref = -HH @ dx.astype(LDE) + r1.astype(LDE) / H2.astype(LDE)
    _check_bound(dx_new, dref, 4 * (n + 4) * U * (aHH @ np.abs(dx) + np.abs(r1 / H2)), f"dx_new n={n} nn={nn}")
