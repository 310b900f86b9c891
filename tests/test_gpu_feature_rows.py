"""Stage tests of the feature-row kernel (be_feature.hip: k_feature_rows<true> / <false>, k_stack_rows, k_triangulate as the row
kernel consumes it) through lvk_ekf_feature_rows, which launches them as the filter does.

Every job is held to the long-double restatement of the reference's formulas in tests/feature_rows_ref.py (checked against the
oracle on the CPU by tests/test_oracle_feature_rows_ref.py).  The projected rows depend on the null-space basis, so only
basis-free quantities are compared:
  - G'^T G' and G'^T r' (G' = the output rows of the compact block, r' their residuals) componentwise within
    C_GRAM / 2 (e_i |g_j| + |g_i| e_j) with e_j = (m nf + K_JAC) u |g_j| + 4 K_JAC u |rho|  (m = 2M raw rows, nf = 3 or 1
    Householder steps, K_JAC = 16, C_GRAM = 2, u = 2^-53, rho = the largest entry of every raw row).  Householder reflections are
    normwise backward stable column by column: the computed column is Q^T (g_j + dg_j) with |dg_j| <= nf c m u |g_j| (Higham,
    Thm 19.4); a Jacobian entry carries at most K_JAC roundings of terms as large as its row (jac_bound); the Gram entry then moves
    by at most e_i |g_j| + |g_i| e_j.  The scale is |g_i| |g_j| and not (|G|^T |G|)_ij: two clones' columns have disjoint
    supports, so (|G|^T |G|)_ij = 0 while the projection makes (G'^T G')_ij non-zero.  For G'^T r' the residual's scale is
    | |r| + |z| |: r = z - p_c / p_c[2] is a difference, its rounding follows |z|, not |r|.
  - |h2| = |H_f| for EKF_NEW within 4 m u |H_f|, and h2 times the range row = H_f^T [G | r] within the Gram bound;
  - gamma within C_GAMMA (k + c) u kappa_2(S) gamma + 2 sqrt(gamma / lambda_min(S)) |dr'| (k gate rows, c compact columns,
    C_GAMMA = 4, |dr'| the bound on the residual's error above): the first-order perturbation of r'^T S^-1 r' by relative
    errors of size (k + c) u in S and by the rounding of r'.
The worst observed ratio to each bound is printed after the module (the _report_worst_ratios fixture) and recorded in PARITY.md.

Exact checks: EKF_TRACKED rows (not projected) componentwise against the restatement, and for if_fej 0 bit-identical to
lvo_be.ekf1d_obs_jacobian; column 6 exactly zero without td; the column map; P NaN outside the union of the jobs' touched blocks
(a wrong column turns gamma non-finite).  Identities between paths: SMALL and general kernel give the same bits except gamma;
fixed-stride and packed observations, direct output, device-zeroed and host-filtered stacking give the same bits; rejected jobs
give zero rows and a zero residual; nothing outside the written dense rows changes (ldh padding included); a tri_pending landmark
gives the bits of the p_w lvk_triangulate returns; a failed triangulation rejects the job."""
import numpy as np
import pytest
from tests import feature_rows_ref as F

pytestmark = pytest.mark.gpu
SIGMA2 = 0.008 ** 2
WORST = {"gram": 0.0, "gamma": 0.0, "h2": 0.0, "tracked": 0.0}


def _lv():
    from larvio_amd import larvio as lv
    return lv


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _spd(rng, n, decades=10.0):
    """SPD, exactly symmetric, variances over `decades` orders of magnitude"""
    B = rng.normal(0, 1, (n, 24))
    C = B @ B.T + np.diag(rng.uniform(4.0, 40.0, n))
    d = 1.0 / np.sqrt(np.diag(C))
    s = 10.0 ** rng.uniform(-1.0 - decades / 2, -1.0, n)
    P = C * (d * s)[:, None] * (d * s)[None, :]
    return (P + P.T) / 2.0


def _ratio(err, bound):
    err = np.asarray(err, np.float64); bound = np.asarray(bound, np.float64)
    out = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return out


def _worst(key, r):
    WORST[key] = max(WORST[key], float(np.max(r)) if np.size(r) else 0.0)


class Batch:
    """jobs + observations + the reference's view of each job"""

    def __init__(self, seed, n_clones, leg=22, n_feat=4):
        self.rng = np.random.default_rng(seed)
        self.clones = F.window(seed, n_clones)
        self.leg = leg; self.n_clones = n_clones
        self.N = leg + 6 * n_clones + n_feat
        self.jobs = []; self.ranks = []; self.z = []; self.zv = []; self.cams = []; self.obs = []
        self.n_new = 0

    def _obs(self, ranks, p_w, noise):
        off = len(self.ranks)
        for r in ranks:
            zz = F.project(self.clones[r], p_w)[0] + self.rng.normal(0, noise, 2)
            R, t = F.cam_pose(self.clones[r])
            self.ranks.append(int(r)); self.z.append(zz); self.zv.append(self.rng.normal(0, 0.05, 2)); self.cams.append((R.ravel(), t))
        return off

    def _ranks(self, M, exclude=()):
        pool = np.setdiff1d(np.arange(self.n_clones), np.array(exclude, int))
        return np.sort(self.rng.choice(pool, M, replace=False))

    def msckf(self, M, noise=0.002, gate=True, tri_pending=0, flip=False):
        lv = _lv(); j = np.zeros((), lv.FEATURE_JOB)
        ranks = self._ranks(M); p_w = F.landmark(self.rng, self.clones)
        j["type"] = lv.FJ_MSCKF; j["n_obs"] = M; j["obs_off"] = self._obs(ranks, p_w, noise)
        if flip:                                                          # behind the cameras: the triangulation fails
            for k in range(M):
                self.z[j["obs_off"] + k] = -self.z[j["obs_off"] + k]
        j["gate"] = 2 * M - 3 if gate else 0; j["tri_pending"] = tri_pending
        j["p_w"] = p_w; j["p_fej"] = p_w + self.rng.normal(0, 1e-3, 3); j["inv_depth"] = 0.25; j["obs_anchor"] = [0, 0, 1]
        self.jobs.append(j)
        return j

    def ekf(self, typ, M, gate, noise=0.002, fcol=None):
        lv = _lv(); j = np.zeros((), lv.FEATURE_JOB)
        anchor = int(self.rng.integers(self.n_clones))
        ranks = self._ranks(M, exclude=(anchor,)); p_w = F.landmark(self.rng, self.clones)
        _, pca = F.project(self.clones[anchor], p_w)
        idp = 1 / pca[2]
        j["type"] = typ; j["n_obs"] = M; j["obs_off"] = self._obs(ranks, p_w, noise); j["anchor_rank"] = anchor
        if fcol is None:
            fcol = self.leg + 6 * self.n_clones + (self.n_new % 4) if gate else self.N + self.n_new
            self.n_new += 1
        j["fcol"] = fcol
        j["gate"] = (2 * M - (1 if typ == lv.FJ_EKF_NEW else 0)) if gate else 0
        j["p_w"] = p_w; j["p_fej"] = p_w + self.rng.normal(0, 1e-3, 3); j["inv_depth"] = idp; j["obs_anchor"] = [pca[0] * idp, pca[1] * idp, 1.0]
        self.jobs.append(j)
        return j

    def arrays(self):
        cams = np.zeros(len(self.cams), np.dtype([("R", np.float64, 9), ("t", np.float64, 3)]))
        for k, (R, t) in enumerate(self.cams):
            cams[k]["R"] = R; cams[k]["t"] = t
        return (np.array(self.jobs), np.array(self.ranks, np.int32), np.array(self.z, np.float64).reshape(-1, 2),
                np.array(self.zv, np.float64).reshape(-1, 2), cams)

    def job_ranks(self, j):
        return self.ranks[int(j["obs_off"]):int(j["obs_off"]) + int(j["n_obs"])]

    def cols(self, j):
        return F.column_map(j, self.job_ranks(j), self.leg)

    def P(self, ldp=None, poison=True, P=None):
        """SPD P (N x N) in an ldp-wide buffer; with poison, NaN outside the union of the gated jobs' touched blocks and in the padding"""
        ldp = ldp or self.N + 3
        if P is None:
            P = _spd(self.rng, self.N)
        buf = np.full((self.N, ldp), np.nan)
        if poison:
            keep = np.zeros((self.N, self.N), bool)
            for j in self.jobs:
                c = self.cols(j); c = c[c < self.N]
                keep[np.ix_(c, c)] = True
            buf[:, :self.N] = np.where(keep, P, np.nan)
        else:
            buf[:, :self.N] = P
        return buf, P

    def run(self, ctx, Pbuf, mode=0, if_fej=1, estimate_td=1, sigma2=SIGMA2, extra_rows=3, ldh=None, cams=False):
        lv = _lv()
        jobs, ranks, z, zv, cm = self.arrays()
        cand = sum(2 * int(j["n_obs"]) - (3 if j["type"] == lv.FJ_MSCKF else 0) for j in jobs if j["type"] != lv.FJ_EKF_NEW)
        H = np.full((cand + extra_rows, ldh or self.N + 5), np.nan); r = np.full(cand + extra_rows, np.nan)
        out = lv.feature_rows(ctx, self.clones, jobs, ranks, z, zv, Pbuf, ldp=Pbuf.shape[1],
                              leg_dim=self.leg, if_fej=if_fej, estimate_td=estimate_td, sigma2=sigma2, mode=mode, cams=cm if cams else None, H=H, r=r)
        return out

    # ---------------------------------------------------------------- reference checks of one job
    def check(self, k, res, block, cc, P, if_fej, estimate_td, sigma2=SIGMA2, gamma_ref=True):
        lv = _lv(); j = self.jobs[k]; typ = int(j["type"]); M = int(j["n_obs"])
        ranks = self.job_ranks(j); z = np.array(self.z[int(j["obs_off"]):int(j["obs_off"]) + M]); zv = np.array(self.zv[int(j["obs_off"]):int(j["obs_off"]) + M])
        G, Hf, rr = F.compact_block(self.clones, j, ranks, z, zv, if_fej, estimate_td)
        c = G.shape[1]
        first = {lv.FJ_MSCKF: 3, lv.FJ_EKF_NEW: 1, lv.FJ_EKF_TRACKED: 0}[typ]
        assert (res["c"], res["rows"], res["first_row"]) == (c, 2 * M - first, first), (k, res)
        assert np.array_equal(cc, self.cols(j)), f"job {k}: column map {cc} != {self.cols(j)}"
        Gk = block[:, :c]; rk = block[:, c]
        assert np.isfinite(block).all(), f"job {k}: non-finite entries at {np.argwhere(~np.isfinite(block))[:4]}"
        if not estimate_td:
            assert not Gk[:, 6].any(), f"job {k}: td column written without estimate_td"
        if typ == lv.FJ_EKF_TRACKED:
            rt = _ratio(np.abs(Gk - np.asarray(G, np.float64)), F.jac_bound(np.asarray(G, np.float64)))
            rz = _ratio(np.abs(rk - np.asarray(rr, np.float64)), F.jac_bound(np.asarray(rr, np.float64)[:, None], (np.abs(z) + 1.0).reshape(-1, 1))[:, 0])
            _worst("tracked", np.concatenate([rt.ravel(), rz]))
            assert rt.max() <= 1 and rz.max() <= 1, f"job {k}: tracked rows off the reference at {np.unravel_index(np.argmax(rt), rt.shape)} (ratio {rt.max():.3g})"
            Hp = None
        else:
            Gp = Gk[first:].astype(F.LD); rp = rk[first:].astype(F.LD)
            if typ == lv.FJ_EKF_NEW:
                assert not Gk[1:, c - 1].any(), f"job {k}: feature column of the null rows not zeroed"
                nf = np.sqrt(float(np.sum(np.asarray(Hf, np.float64) ** 2)))
                rh = abs(abs(res["h2"]) - nf) / (4 * 2 * M * F.U * nf)
                _worst("h2", rh)
                assert rh <= 1 and Gk[0, c - 1] == res["h2"], (k, res["h2"], nf)
                # the range row: h2 [G | r]_0 = H_f^T [G | r]
                lhs = res["h2"] * np.concatenate([Gk[0, :c - 1], [rk[0]]]).astype(F.LD)
                rhs = np.concatenate([Hf[:, 0] @ G[:, :c - 1], [Hf[:, 0] @ rr]])
                bnd = np.concatenate([F.gram_bound(G, Hf)[c - 1, :c - 1], F.gram_bound(G, Hf, F.residual_scale(rr, z))[c - 1]])
                rr0 = _ratio(np.abs(np.asarray(lhs - rhs, np.float64)), bnd)
                _worst("gram", rr0)
                assert rr0.max() <= 1, f"job {k}: range row off at column {int(np.argmax(rr0))} (ratio {rr0.max():.3g})"
            GtG, Gtr = F.projected_grams(G, Hf, rr)
            e1 = _ratio(np.abs(np.asarray(Gp.T @ Gp - GtG, np.float64)), F.gram_bound(G, Hf))
            e2 = _ratio(np.abs(np.asarray(Gp.T @ rp - Gtr, np.float64)), F.gram_bound(G, Hf, F.residual_scale(rr, z))[:, 0])
            _worst("gram", np.concatenate([e1.ravel(), e2]))
            assert e1.max() <= 1, f"job {k}: G'^T G' off at {np.unravel_index(np.argmax(e1), e1.shape)} (ratio {e1.max():.3g})"
            assert e2.max() <= 1, f"job {k}: G'^T r' off at {int(np.argmax(e2))} (ratio {e2.max():.3g})"
            Hp = Hf
        if int(j["gate"]) and gamma_ref:
            cols = self.cols(j)
            Pcc = P[np.ix_(cols, cols)]
            g = F.gate_gamma(G, Hp, rr, Pcc, sigma2)
            b = F.gamma_bound(G, Hp, Pcc, sigma2, g, F.residual_scale(rr, z))
            rg = abs(res["gamma"] - float(g)) / b
            _worst("gamma", rg)
            assert np.isfinite(res["gamma"]) and rg <= 1, f"job {k}: gamma {res['gamma']!r} vs {float(g)!r} (ratio {rg:.3g})"
            thr = _lvk_thr(int(j["gate"]))
            assert bool(res["accept"]) == (res["gamma"] < thr)
            if abs(float(g) - thr) > b:
                assert bool(res["accept"]) == (float(g) < thr), (k, float(g), thr)
        elif not int(j["gate"]):
            assert res["gamma"] == 0.0 and res["accept"] == 1


def _lvk_thr(dof):
    from oracle import lvo_be
    return lvo_be.chi2_table(dof)            # the table lvk_chi2_005 holds (larvio.cpp:353-357: dof 1..99, 0 beyond)


def _check_dense(b, out, mode_slots=True):
    """dense rows as the jobs' blocks dictate: accepted -> the compact rows scattered, rejected -> zero row and zero residual;
    everything else of the buffer (rows past the end, the ldh padding) still NaN"""
    lv = _lv()
    res, blocks, ccs, H, r, rows = out
    N = b.N
    Hexp = np.full(H.shape, np.nan); rexp = np.full(r.shape, np.nan)
    d0 = 0
    for k, j in enumerate(b.jobs):
        if j["type"] == lv.FJ_EKF_NEW:
            continue
        first = 3 if j["type"] == lv.FJ_MSCKF else 0
        n = 2 * int(j["n_obs"]) - first
        if not mode_slots and not res[k]["accept"]:
            continue
        Hexp[d0:d0 + n, :N] = 0.0; rexp[d0:d0 + n] = 0.0
        if res[k]["accept"]:
            c = int(res[k]["c"]); cc = ccs[k]
            for a in range(n):
                for q in range(c):
                    if cc[q] < N:
                        Hexp[d0 + a, cc[q]] = blocks[k][first + a, q]
                rexp[d0 + a] = blocks[k][first + a, c]
        d0 += n
    assert rows == d0
    bad = _bits(H) != _bits(Hexp)
    assert not bad.any(), f"dense H differs at {np.argwhere(bad)[:4].tolist()}"
    assert np.array_equal(_bits(r), _bits(rexp)), f"dense r differs at {np.argwhere(_bits(r) != _bits(rexp))[:4].tolist()}"


def _same_blocks(a, b, gamma=True):
    for k in range(len(a[0])):
        for f in ("h2", "rows", "first_row", "c", "accept") + (("gamma",) if gamma else ()):
            assert _bits(np.float64(a[0][k][f])) == _bits(np.float64(b[0][k][f])), (k, f, a[0][k][f], b[0][k][f])
        assert np.array_equal(_bits(a[1][k]), _bits(b[1][k])), f"job {k}: [G | r] differs at {np.argwhere(_bits(a[1][k]) != _bits(b[1][k]))[:4].tolist()}"
        assert np.array_equal(a[2][k], b[2][k])


# ==================================================================== shapes
@pytest.mark.parametrize("M", [2, 3, 7, 8, 9, 20, 33, 63, 64])
def test_msckf_rows_and_gate(gpu_ctx, M):
    """MSCKF jobs: 8 is the SMALL kernel's largest (k = 13), 9 the first general one, 64 gives 128 rows (= FR_THREADS) and ~136 KB of LDS"""
    lv = _lv()
    n_clones = min(64, max(M + 2, 12))
    fej, td = M % 2, (M // 2) % 2
    b = Batch(1000 + M, n_clones)
    for _ in range(3):
        b.msckf(M)
    Pbuf, P = b.P()
    out = b.run(gpu_ctx, Pbuf, if_fej=fej, estimate_td=td)
    for k in range(3):
        b.check(k, out[0][k], out[1][k], out[2][k], P, fej, td)
    _check_dense(b, b.run(gpu_ctx, Pbuf, mode=lv.FR_DIRECT, if_fej=fej, estimate_td=td))
    if M <= 8:                                                            # the SMALL batch against the general kernel: same rows, gamma within the bound
        g = b.run(gpu_ctx, Pbuf, mode=lv.FR_GENERAL, if_fej=fej, estimate_td=td)
        _same_blocks(out, g, gamma=False)
        for k in range(3):
            b.check(k, g[0][k], g[1][k], g[2][k], P, fej, td)
        _same_blocks(out, b.run(gpu_ctx, Pbuf, mode=lv.FR_STRIDE, if_fej=fej, estimate_td=td))


@pytest.mark.parametrize("M,gate", [(1, False), (2, False), (7, False), (8, False), (7, True), (8, True)])
def test_ekf_new_rows(gpu_ctx, M, gate):
    """a new in-state feature: one Householder step on its feature column, the range row h2.  M = 8 gives c = 62 (FRS_COLS 64);
    gated at M = 7 and 8: k = 13 and 15, the full 16x16 MFMA tile of the SMALL gate"""
    lv = _lv()
    for fej, td in ((1, 1), (0, 0)):
        b = Batch(2000 + 10 * M + gate, 14)
        for _ in range(2):
            b.ekf(lv.FJ_EKF_NEW, M, gate)
        Pbuf, P = b.P()
        out = b.run(gpu_ctx, Pbuf, if_fej=fej, estimate_td=td)
        for k in range(2):
            b.check(k, out[0][k], out[1][k], out[2][k], P, fej, td)
        assert out[5] == 0 and np.isnan(out[3]).all()                     # EKF_NEW rows never reach the dense matrix
        g = b.run(gpu_ctx, Pbuf, mode=lv.FR_GENERAL, if_fej=fej, estimate_td=td)
        _same_blocks(out, g, gamma=not gate)
        for k in range(2):
            b.check(k, g[0][k], g[1][k], g[2][k], P, fej, td)


@pytest.mark.parametrize("M", [1, 8])
def test_ekf_tracked_rows(gpu_ctx, M):
    """a tracked in-state feature: raw rows, gated.  M = 8 gives 16 gate rows, which the shared routing rule must send to the
    general kernel (the SMALL tile holds 15)"""
    lv = _lv()
    from oracle import lvo_be
    for fej, td in ((1, 1), (0, 1), (1, 0), (0, 0)):
        b = Batch(3000 + M, 12)
        for _ in range(3):
            b.ekf(lv.FJ_EKF_TRACKED, M, True)
        Pbuf, P = b.P()
        out = b.run(gpu_ctx, Pbuf, if_fej=fej, estimate_td=td)
        for k in range(3):
            b.check(k, out[0][k], out[1][k], out[2][k], P, fej, td)
        if M == 8:
            _same_blocks(out, b.run(gpu_ctx, Pbuf, mode=lv.FR_GENERAL, if_fej=fej, estimate_td=td))
        # all 2M rows of a tracked job reach the dense matrix, in every output mode
        _check_dense(b, out, mode_slots=False)
        for mode in (lv.FR_DIRECT, lv.FR_DEVICE_ZERO):
            o = b.run(gpu_ctx, Pbuf, mode=mode, if_fej=fej, estimate_td=td)
            _same_blocks(out, o)
            _check_dense(b, o)
        if not fej:                                                       # be_dev.h: the device Jacobian is the oracle's, bit for bit
            for k, j in enumerate(b.jobs):
                ca = b.clones[int(j["anchor_rank"])]; c = int(out[0][k]["c"])
                for t, rk in enumerate(b.job_ranks(j)):
                    zz = b.z[int(j["obs_off"]) + t]
                    ok, Hf, Ha, Hx, He, r = lvo_be.ekf1d_obs_jacobian(b.clones[rk], ca, j["p_w"], j["inv_depth"], j["obs_anchor"], zz)
                    blk = out[1][k][2 * t:2 * t + 2]
                    assert np.array_equal(_bits(blk[:, 0:6]), _bits(He)) and np.array_equal(_bits(blk[:, 7:13]), _bits(Ha))
                    assert np.array_equal(_bits(blk[:, 13 + 6 * t:19 + 6 * t]), _bits(Hx)) and np.array_equal(_bits(blk[:, c - 1]), _bits(Hf))
                    assert np.array_equal(_bits(blk[:, c]), _bits(r))


@pytest.mark.parametrize("leg,n_clones,fej,td", [(22, 20, 1, 1), (22, 20, 0, 1), (22, 20, 1, 0), (22, 20, 0, 0), (46, 16, 1, 1), (22, 64, 1, 1)])
def test_mixed_batch_all_paths(gpu_ctx, leg, n_clones, fej, td):
    """all three job types in one launch, ordered as the filter orders them (backend.hip: [new: msckf-form gate | new: ekf rows]
    [tracked] [msckf]), some rejected.  n_clones 64 puts the SMALL kernel's clone table at ~98 % of the 64 KB LDS line.  Every mode
    gives the same bits; every job matches the reference."""
    lv = _lv()
    b = Batch(4000 + leg + n_clones + 2 * fej + td, n_clones, leg=leg)
    for _ in range(2):
        b.msckf(6); b.ekf(lv.FJ_EKF_NEW, 5, False)
    for k in range(4):
        b.ekf(lv.FJ_EKF_TRACKED, 1, True, noise=0.0003 if k % 2 == 0 else 0.05)
    for k in range(5):
        b.msckf(int(b.rng.integers(3, 9)), noise=0.0005 if k != 2 else 0.05)
    Pbuf, P = b.P()
    base = b.run(gpu_ctx, Pbuf, if_fej=fej, estimate_td=td)
    for k in range(len(b.jobs)):
        b.check(k, base[0][k], base[1][k], base[2][k], P, fej, td)
    acc = [bool(x["accept"]) for x in base[0]]
    assert not all(acc) and sum(acc) > len(acc) // 2
    _check_dense(b, base, mode_slots=False)
    outs = {m: b.run(gpu_ctx, Pbuf, mode=m, if_fej=fej, estimate_td=td) for m in (lv.FR_STRIDE, lv.FR_DIRECT, lv.FR_DEVICE_ZERO, lv.FR_STRIDE | lv.FR_DIRECT)}
    for m, o in outs.items():
        _same_blocks(base, o)
    _check_dense(b, outs[lv.FR_DIRECT]); _check_dense(b, outs[lv.FR_DEVICE_ZERO]); _check_dense(b, outs[lv.FR_STRIDE | lv.FR_DIRECT])
    assert np.array_equal(_bits(outs[lv.FR_DIRECT][3]), _bits(outs[lv.FR_DEVICE_ZERO][3])) and np.array_equal(_bits(outs[lv.FR_DIRECT][4]), _bits(outs[lv.FR_DEVICE_ZERO][4]))
    g = b.run(gpu_ctx, Pbuf, mode=lv.FR_GENERAL | lv.FR_DIRECT, if_fej=fej, estimate_td=td)
    _same_blocks(base, g, gamma=False)
    for k in range(len(b.jobs)):
        b.check(k, g[0][k], g[1][k], g[2][k], P, fej, td)


# ==================================================================== gate decisions and edges
def _sigma2_at(b, k, P, fej, td, target):
    """sigma2 with gamma_ref(sigma2) = target (gamma falls as sigma2 grows), by bisection in log sigma2, long double"""
    j = b.jobs[k]; M = int(j["n_obs"])
    z = np.array(b.z[int(j["obs_off"]):int(j["obs_off"]) + M]); zv = np.array(b.zv[int(j["obs_off"]):int(j["obs_off"]) + M])
    G, Hf, rr = F.compact_block(b.clones, j, b.job_ranks(j), z, zv, fej, td)
    Hp = None if int(j["type"]) == 2 else Hf
    cols = b.cols(j); Pcc = P[np.ix_(cols, cols)]
    lo, hi = F.LD(-30), F.LD(5)
    for _ in range(90):
        mid = (lo + hi) / 2
        if F.gate_gamma(G, Hp, rr, Pcc, float(np.exp(mid))) > target:
            lo = mid
        else:
            hi = mid
    return float(np.exp((lo + hi) / 2))


@pytest.mark.parametrize("kind", ["msckf", "tracked", "new8"])
def test_gate_decision_at_the_threshold(gpu_ctx, kind):
    """sigma2 chosen so that the reference's gamma is thr (1 -+ 1e-7): both kernels accept, respectively reject, as the reference does"""
    lv = _lv()
    b = Batch(5000 + len(kind), 12)
    if kind == "msckf":
        b.msckf(5, noise=0.01)
    elif kind == "tracked":
        b.ekf(lv.FJ_EKF_TRACKED, 1, True, noise=0.01)
    else:
        b.ekf(lv.FJ_EKF_NEW, 8, True, noise=0.01)
    Pbuf, P = b.P()
    thr = _lvk_thr(int(b.jobs[0]["gate"]))
    for f, want in ((1 - 1e-7, 1), (1 + 1e-7, 0)):
        s2 = _sigma2_at(b, 0, P, 1, 1, thr * f)
        for mode in (0, lv.FR_GENERAL):
            out = b.run(gpu_ctx, Pbuf, mode=mode, sigma2=s2)
            assert out[0][0]["accept"] == want, (kind, mode, f, out[0][0]["gamma"], thr)
            b.check(0, out[0][0], out[1][0], out[2][0], P, 1, 1, sigma2=s2)


@pytest.mark.parametrize("kind", ["msckf", "tracked"])
def test_non_positive_pivot_rejects(gpu_ctx, kind):
    """P negative definite on the touched block, sigma2 tiny: no Cholesky exists, both paths give gamma = 1e300 and reject"""
    lv = _lv()
    b = Batch(6000 + len(kind), 10)
    b.msckf(4) if kind == "msckf" else b.ekf(lv.FJ_EKF_TRACKED, 1, True)
    Pbuf, P = b.P(P=-_spd(np.random.default_rng(1), b.N))
    for mode in (0, lv.FR_GENERAL):
        out = b.run(gpu_ctx, Pbuf, mode=mode, sigma2=1e-30)
        assert out[0][0]["gamma"] == 1e300 and out[0][0]["accept"] == 0, (mode, out[0][0])


# ==================================================================== triangulation consumed on the device
def test_tri_pending_matches_host_triangulation(gpu_ctx):
    """FJ_TRI_PENDING: the landmark comes from k_triangulate's result slot.  Same bits as passing the p_w lvk_triangulate returns;
    a failed triangulation (landmark behind the cameras) rejects the job with zero rows"""
    lv = _lv()
    b = Batch(7000, 16)
    for k in range(5):
        b.msckf(int(3 + k), tri_pending=1, flip=(k == 3))
    Pbuf, P = b.P()
    pend = b.run(gpu_ctx, Pbuf, mode=lv.FR_DIRECT, cams=True)
    jobs, ranks, z, zv, cams = b.arrays()
    for k, j in enumerate(b.jobs):
        o = int(j["obs_off"]); M = int(j["n_obs"])
        ok, pos, *_ = lv.triangulate(gpu_ctx, cams[o:o + M], z[o:o + M])
        assert ok == (k != 3)
        if ok:
            j["p_w"] = pos
        j["tri_pending"] = 0
    host = b.run(gpu_ctx, Pbuf, mode=lv.FR_DIRECT)
    for k in range(len(b.jobs)):
        if k == 3:
            assert pend[0][k]["accept"] == 0
            continue
        for f in ("gamma", "h2", "rows", "first_row", "c", "accept"):
            assert _bits(np.float64(pend[0][k][f])) == _bits(np.float64(host[0][k][f])), (k, f)
        assert np.array_equal(_bits(pend[1][k]), _bits(host[1][k]))
        b.check(k, pend[0][k], pend[1][k], pend[2][k], P, 1, 1)
    _check_dense(b, pend)
    rows3 = slice(sum(2 * int(b.jobs[q]["n_obs"]) - 3 for q in range(3)), sum(2 * int(b.jobs[q]["n_obs"]) - 3 for q in range(4)))
    assert not pend[3][rows3, :b.N].any() and not pend[4][rows3].any()


# ==================================================================== ties to the older entry and host checks
def test_flat_batch_equals_gate_and_stack(gpu_ctx):
    """the batch of test_gate_and_stack_stage_matches_oracle through both entries: the same rows and gamma, bit for bit"""
    lv = _lv()
    from tests.test_oracle_backend import _scene
    n_clones = 12; N = 22 + 6 * n_clones + 4
    rng = np.random.default_rng(77)
    Bm = rng.normal(0, 1, (N, N)); P = Bm @ Bm.T * 2e-6 + np.eye(N) * 1e-7
    clones = None; feats = []; ranks_all = []; obs_all = []; vel_all = []
    for k, (seed, M) in enumerate(((2, 6), (3, 3), (4, 12), (6, 2), (8, 9))):
        c, ranks, obs, vel, p_w, from_q = _scene(seed, M=M, n_clones=n_clones)
        if clones is None:
            clones = c
        else:
            for j, r in enumerate(ranks):
                pc = from_q(clones[r]["q_cam"]).T @ (p_w - clones[r]["p_cam"])
                obs[j] = pc[:2] / pc[2] + rng.normal(0, 0.004 * (1 + 3 * (k == 2)), 2)
        feats.append((p_w, M, len(ranks_all)))
        ranks_all += list(ranks); obs_all += list(obs); vel_all += list(vel)
    obs_all = np.array(obs_all); vel_all = np.array(vel_all)
    Hg, rg, gamma, acc = lv.gate_and_stack(gpu_ctx, clones, feats, ranks_all, obs_all, vel_all, P, 0.008 ** 2)
    jobs = np.zeros(len(feats), lv.FEATURE_JOB)
    for k, (pw, M, off) in enumerate(feats):
        jobs[k]["type"] = lv.FJ_MSCKF; jobs[k]["n_obs"] = M; jobs[k]["obs_off"] = off; jobs[k]["gate"] = 2 * M - 3
        jobs[k]["p_w"] = pw; jobs[k]["p_fej"] = pw; jobs[k]["inv_depth"] = 1.0
    res, blocks, ccs, H, r, rows = lv.feature_rows(gpu_ctx, clones, jobs, ranks_all, obs_all, vel_all, P, sigma2=0.008 ** 2)
    assert np.array_equal(_bits(res["gamma"]), _bits(gamma)) and np.array_equal(res["accept"].astype(bool), acc)
    assert rows == Hg.shape[0]
    assert np.array_equal(_bits(H[:rows]), _bits(Hg)) and np.array_equal(_bits(r[:rows]), _bits(rg))


def test_bad_input_is_refused(gpu_ctx):
    """host checks: nothing is launched for input the kernel does not handle"""
    lv = _lv()
    b = Batch(8000, 10)
    b.msckf(3); b.ekf(lv.FJ_EKF_TRACKED, 1, True)
    Pbuf, P = b.P(poison=False)
    jobs, ranks, z, zv, cams = b.arrays()

    def call(jobs=jobs, ranks=ranks, mode=0, leg=22):
        return lv.feature_rows(gpu_ctx, b.clones, jobs, ranks, z, zv, Pbuf, leg_dim=leg, mode=mode)

    call()
    ARG, CAP = "lvk status 1: ", "lvk status 3: "
    for field, val, msg in (("n_obs", 0, "0 observations"), ("n_obs", 65, "65 observations"), ("type", 3, "unknown type 3"), ("gate", -1, "bad gate")):
        bad = jobs.copy(); bad[1][field] = val
        with pytest.raises(lv.LvkError, match=ARG + ".*" + msg):
            call(bad)
    bad = jobs.copy(); bad[0]["n_obs"] = 1                               # MSCKF needs two views
    with pytest.raises(lv.LvkError, match=ARG + "job 0: 1 observations"):
        call(bad)
    bad = jobs.copy(); bad[1]["anchor_rank"] = int(ranks[int(bad[1]["obs_off"])])      # the anchor observes the feature
    with pytest.raises(lv.LvkError, match=ARG + "job 1: the anchor clone .* is also an observing clone"):
        call(bad)
    bad = jobs.copy(); bad[1]["fcol"] = 5                                # the feature column must be a feature state
    with pytest.raises(lv.LvkError, match=ARG + "job 1: feature column 5"):
        call(bad)
    rk = ranks.copy(); rk[0] = 10
    with pytest.raises(lv.LvkError, match=ARG + "job 0: clone rank 10 out of range"):
        call(ranks=rk)
    rk = ranks.copy(); rk[1] = rk[0]
    with pytest.raises(lv.LvkError, match=ARG + "job 0: clone rank .* observed twice"):
        call(ranks=rk)
    with pytest.raises(lv.LvkError, match=ARG + ".*exclude each other"):
        call(mode=lv.FR_DIRECT | lv.FR_DEVICE_ZERO)
    with pytest.raises(lv.LvkError, match=ARG + ".*leg_dim 30"):
        call(leg=30)
    for mode in (0, lv.FR_DIRECT, lv.FR_DEVICE_ZERO):                   # every candidate row must fit, whichever the mode
        with pytest.raises(lv.LvkError, match=CAP + ".*exceed h_rows"):
            lv.feature_rows(gpu_ctx, b.clones, jobs, ranks, z, zv, Pbuf, mode=mode, H=np.full((4, b.N), np.nan))
    call()                                                                # the context is still usable


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """after the module: the worst observed ratio to each bound (recorded in PARITY.md).  A report only - every check asserts its
    own ratio <= 1 where it is computed."""
    yield
    print("\nworst ratio to bound:", {k: f"{v:.3e}" for k, v in WORST.items()})
