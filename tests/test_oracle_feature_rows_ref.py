"""CPU: the long-double restatement of the feature rows (tests/feature_rows_ref.py) against the oracle's featureJacobian_msckf,
gatingTest and measurementJacobian_ekf_1didp, within the bounds the GPU stage tests use, so that the reference is trusted before
any GPU run.  The oracle's stage entry for the 1-D inverse-depth Jacobian has no FEJ variant: the FEJ branch of the restatement
is held to it only where both branches must agree (FEJ points equal to the current ones), test_ekf1d_fej_branch_at_consistent_points;
a wrong FEJ point in that branch (which point feeds which term) is checked only against the kernel on the GPU."""
import numpy as np
import pytest
from oracle import lvo_be
from tests import feature_rows_ref as F

SIGMA2 = 0.008 ** 2


def _P(rng, N):
    """SPD with variances over ten decades (as tests/test_gpu_covariance_ops.py)"""
    B = rng.normal(0, 1, (N, N)) * 0.3
    d = 10.0 ** rng.uniform(-10, 0, N)
    P = (B @ B.T + np.eye(N)) * np.sqrt(np.outer(d, d)) * 1e-2
    return (P + P.T) / 2


@pytest.mark.parametrize("M,n_clones,if_fej,estimate_td,leg", [(2, 8, 1, 1, 22), (3, 8, 0, 1, 22), (7, 12, 1, 0, 22), (8, 10, 1, 1, 46),
                                                                 (12, 14, 0, 0, 22), (20, 24, 1, 1, 22), (33, 40, 1, 1, 46)])
def test_msckf_restatement_matches_oracle(M, n_clones, if_fej, estimate_td, leg):
    rng = np.random.default_rng(M * 100 + n_clones)
    clones = F.window(M + n_clones, n_clones)
    p_w = F.landmark(rng, clones)
    ranks = np.sort(rng.choice(n_clones, M, replace=False)).astype(np.int32)
    z = np.array([F.project(clones[r], p_w)[0] + rng.normal(0, 0.003, 2) for r in ranks]); zv = rng.normal(0, 0.05, (M, 2))
    N = leg + 6 * n_clones + 3
    H, r = lvo_be.msckf_feature_jacobian(clones, ranks, z, zv, p_w, N, leg_dim=leg, if_fej=if_fej, estimate_td=estimate_td)
    job = {"type": 0, "n_obs": M, "p_w": p_w}
    G, Hf, rr = F.compact_block(clones, job, ranks, z, zv, if_fej, estimate_td)
    cols = F.column_map(job, ranks, leg)
    other = np.setdiff1d(np.arange(N), cols)
    assert not H[:, other].any()                                        # nothing outside the compact columns
    Hc = H[:, cols].astype(F.LD)
    GtG, Gtr = F.projected_grams(G, Hf, rr)
    e1 = np.abs(np.asarray(Hc.T @ Hc - GtG, np.float64)) / F.gram_bound(G, Hf)
    e2 = np.abs(np.asarray(Hc.T @ r.astype(F.LD) - Gtr, np.float64)) / F.gram_bound(G, Hf, F.residual_scale(rr, z))[:, 0]
    e1, e2 = np.where(np.isnan(e1), 0, e1), np.where(np.isnan(e2), 0, e2)            # 0 / 0: an exactly zero column (td off)
    assert e1.max() < 1 and e2.max() < 1, (e1.max(), e2.max())
    P = _P(rng, N)
    g_o = lvo_be.gating_gamma(H, r, P, SIGMA2)
    g_l = F.gate_gamma(G, Hf, rr, P[np.ix_(cols, cols)], SIGMA2)
    bound = F.gamma_bound(G, Hf, P[np.ix_(cols, cols)], SIGMA2, g_l, F.residual_scale(rr, z))
    assert abs(g_o - float(g_l)) < bound, (g_o, float(g_l), abs(g_o - float(g_l)) / bound)
    print(f"M {M}: gram ratio {max(e1.max(), e2.max()):.2e}, gamma ratio {abs(g_o - float(g_l)) / bound:.2e}")


@pytest.mark.parametrize("seed", range(6))
def test_ekf1d_restatement_matches_oracle(seed):
    rng = np.random.default_rng(seed)
    clones = F.window(seed, 10)
    p_w = F.landmark(rng, clones)
    ka, kk = rng.choice(10, 2, replace=False)
    _, pca = F.project(clones[ka], p_w)
    idp = 1 / pca[2]; oa = np.array([pca[0] * idp, pca[1] * idp, 1.0])
    z = F.project(clones[kk], p_w)[0] + rng.normal(0, 0.003, 2)
    ok, Hf, Ha, Hx, He, r = lvo_be.ekf1d_obs_jacobian(clones[kk], clones[ka], p_w, idp, oa, z)
    assert ok
    hf, ha, hx, he, rr = F.ekf_obs(clones[kk], clones[ka], p_w, p_w, idp, oa, z, 0)
    for got, ref, scale in ((Hf, hf, None), (Ha, ha, None), (Hx, hx, None), (He, he, None), (r, rr, np.abs(z) + np.abs(r))):
        ref = np.asarray(ref, np.float64)
        assert (np.abs(got - ref) <= F.jac_bound(ref, scale)).all(), (got, ref)


def test_gamma_matches_oracle_for_the_raw_two_rows():
    """gatingTest on unprojected rows (a tracked in-state feature) with the restated gate"""
    rng = np.random.default_rng(3)
    clones = F.window(3, 10); N = 22 + 60 + 2
    p_w = F.landmark(rng, clones)
    _, pca = F.project(clones[2], p_w); idp = 1 / pca[2]; oa = np.array([pca[0] * idp, pca[1] * idp, 1.0])
    job = {"type": 2, "n_obs": 1, "anchor_rank": 2, "fcol": N - 1, "p_w": p_w, "p_fej": p_w, "inv_depth": idp, "obs_anchor": oa}
    ranks = [9]; z = np.array([F.project(clones[9], p_w)[0] + 0.002]); zv = np.array([[0.01, -0.02]])
    G, _, rr = F.compact_block(clones, job, ranks, z, zv, 0, 1)
    cols = F.column_map(job, ranks, 22)
    H = np.zeros((2, N)); H[:, cols] = np.asarray(G, np.float64)
    P = _P(rng, N)
    g_o = lvo_be.gating_gamma(H, np.asarray(rr, np.float64), P, SIGMA2)
    g_l = F.gate_gamma(G, None, rr, P[np.ix_(cols, cols)], SIGMA2)
    assert abs(g_o - float(g_l)) < F.gamma_bound(G, None, P[np.ix_(cols, cols)], SIGMA2, g_l, F.residual_scale(rr, z))


@pytest.mark.parametrize("seed", range(4))
def test_ekf1d_fej_branch_at_consistent_points(seed):
    """with every FEJ point equal to the current one (clones' p_fej = p, the feature's p_fej = p_w) and obs_anchor / inv_depth taken
    from p_w in the anchor camera, the FEJ branch's p_ca, p_baf and p_bkf equal the plain branch's: the oracle's result applies"""
    rng = np.random.default_rng(100 + seed)
    clones = F.window(100 + seed, 10)
    clones["p_fej"] = clones["p"]
    p_w = F.landmark(rng, clones)
    ka, kk = rng.choice(10, 2, replace=False)
    _, pca = F.project(clones[ka], p_w)
    idp = 1 / pca[2]; oa = np.array([pca[0] * idp, pca[1] * idp, 1.0])
    z = F.project(clones[kk], p_w)[0] + rng.normal(0, 0.003, 2)
    ok, Hf, Ha, Hx, He, r = lvo_be.ekf1d_obs_jacobian(clones[kk], clones[ka], p_w, idp, oa, z)
    assert ok
    hf, ha, hx, he, rr = F.ekf_obs(clones[kk], clones[ka], p_w, p_w, idp, oa, z, 1)
    # the two branches agree up to the rounding of their inputs (obs_anchor and inv_depth are doubles): the scale of an entry is
    # then the size of the terms that cancel in it, |dz/dp_c| (|p_w - p_k| + |p_ca| + 1), not the entry's row
    _, pck = F.project(clones[kk], p_w)
    jk = np.array([1 / abs(pck[2]) + abs(pck[0]) / pck[2] ** 2, 1 / abs(pck[2]) + abs(pck[1]) / pck[2] ** 2])
    s = (jk * (np.linalg.norm(p_w - clones[kk]["p"]) + np.linalg.norm(pca) + 1))[:, None]
    for got, ref, scale in ((Hf, hf, s[:, 0] / idp ** 2), (Ha, ha, s), (Hx, hx, s), (He, he, s), (r, rr, np.abs(z) + np.abs(r))):
        ref = np.asarray(ref, np.float64)
        assert (np.abs(got - ref) <= F.jac_bound(ref, scale)).all(), (got, ref)
