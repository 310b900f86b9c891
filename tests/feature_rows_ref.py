"""Extended-precision restatement of the per-feature measurement rows (numpy longdouble), for the stage tests of k_feature_rows.

Restated from the reference's formulas, not from the kernel's decomposition:
  - measurementJacobian_msckf (larvio.cpp:859-921): dz/dp_c [R_w2c [p_bf]x, -R_w2c] for the clone, dz/dp_c [R_w2c [p_bf]x R_b2w -
    R_b2c [t_c_b]x, -R_b2c] for the extrinsics, dz/dp_c R_w2c for the landmark, p_bf = p_w - p (p_fej under FEJ);
  - measurementJacobian_ekf_1didp (:1117-1244): the same chain through the anchor frame, with p_ca = obs_anchor / rho (or, under
    FEJ, the FEJ landmark expressed in the anchor camera) and d p_ca / d rho = -obs_anchor / rho^2;
  - the left-null-space projection (:924-981, 2095-2119) enters only through quantities that do not depend on the chosen basis A
    of null(H_f^T): G'^T G' = G^T Pi G and G'^T r' = G^T Pi r with Pi = I - H_f (H_f^T H_f)^-1 H_f^T;
  - the gate gamma = r'^T (G' P G'^T + sigma2 I)^-1 r' (:1865-1880) as rW r - b^T (H_f^T W^-1 H_f)^-1 b with W = G P G^T + sigma2 I,
    rW = W^-1 r, b = H_f^T rW (the inverse of A^T W A sandwiched by A, written without A).
Compact column layout (as the kernel's column map names it): MSCKF [extrinsics 6 | td | clone blocks in observation order],
EKF [extrinsics 6 | td | anchor block | clone blocks | feature column].
"""
import numpy as np

LD = np.longdouble
U = np.finfo(np.float64).eps / 2            # unit roundoff of the kernel's arithmetic


def rot(q):
    """[x y z w] -> rotation matrix (Eigen's toRotationMatrix), long double"""
    x, y, z, w = (LD(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=LD)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=LD)


def _v(a):
    return np.asarray(a, np.float64).astype(LD)


def _dz(p):
    return np.array([[1 / p[2], 0, -p[0] / (p[2] * p[2])], [0, 1 / p[2], -p[1] / (p[2] * p[2])]], dtype=LD)


def msckf_obs(clone, p_w, z, if_fej):
    """one observation: (Hx 2x6, He 2x6, Hf 2x3, r 2)"""
    R_b2w = rot(clone["q"]); R_b2c = _v(clone["R_b2c"]).reshape(3, 3); t_c_b = _v(clone["t_c_b"]); p = _v(clone["p"])
    R_w2c = R_b2c @ R_b2w.T
    p_w = _v(p_w)
    p_c = R_w2c @ (p_w - (p + R_b2w @ t_c_b))
    p_bf = p_w - (_v(clone["p_fej"]) if if_fej else p)
    dz = _dz(p_c)
    Hx = dz @ np.hstack([R_w2c @ skew(p_bf), -R_w2c])
    He = dz @ np.hstack([R_w2c @ skew(p_bf) @ R_b2w - R_b2c @ skew(t_c_b), -R_b2c])
    Hf = dz @ R_w2c
    r = _v(z) - p_c[:2] / p_c[2]
    return Hx, He, Hf, r


def ekf_obs(ck, ca, p_w, p_fej, inv_depth, obs_anchor, z, if_fej):
    """one observation of a 1-D inverse-depth feature anchored in clone ca, seen from clone ck != ca: (Hf 2, Ha 2x6, Hx 2x6, He 2x6, r 2)"""
    R_b2c = _v(ck["R_b2c"]).reshape(3, 3); t_c_b = _v(ck["t_c_b"])
    R_bk2w = rot(ck["q"]); R_ba2w = rot(ca["q"])
    R_w2ck = R_b2c @ R_bk2w.T; R_w2ca = R_b2c @ R_ba2w.T
    p_w = _v(p_w); p_fej = _v(p_fej); rho = LD(float(inv_depth)); f_an = _v(obs_anchor)
    if if_fej:
        p_ca = R_b2c @ (R_ba2w.T @ (p_fej - _v(ca["p_fej"])) - t_c_b)
    else:
        p_ca = f_an / rho
    p_ck = R_w2ck @ (p_w - (_v(ck["p"]) + R_bk2w @ t_c_b))
    r = _v(z) - p_ck[:2] / p_ck[2]
    Jk = _dz(p_ck)
    dpck_drho = R_w2ck @ R_w2ca.T @ (-f_an / (rho * rho))
    p_baf = (p_fej - _v(ca["p_fej"])) if if_fej else (p_w - _v(ca["p"]))
    p_bkf = (p_fej - _v(ck["p_fej"])) if if_fej else (p_w - _v(ck["p"]))
    Ha = Jk @ np.hstack([-R_w2ck @ skew(p_baf), R_w2ck])
    Hx = Jk @ np.hstack([R_w2ck @ skew(p_bkf), -R_w2ck])
    RR = R_bk2w.T @ R_ba2w
    Je = np.hstack([R_b2c @ (skew(R_bk2w.T @ p_bkf - t_c_b) - RR @ skew(R_b2c.T @ p_ca)), R_b2c @ (RR - np.eye(3, dtype=LD))])
    He = Jk @ Je
    return Jk @ dpck_drho, Ha, Hx, He, r


def compact_block(clones, job, ranks, z, zv, if_fej, estimate_td):
    """raw compact rows of one job: (G 2M x c, H_f 2M x nf, r 2M).  For EKF jobs the feature column is both G's last column and H_f."""
    M = int(job["n_obs"]); ekf = int(job["type"]) != 0
    c = 7 + 6 + 6 * M + 1 if ekf else 7 + 6 * M
    G = np.zeros((2 * M, c), LD); Hf = np.zeros((2 * M, 1 if ekf else 3), LD); r = np.zeros(2 * M, LD)
    for t in range(M):
        ck = clones[ranks[t]]
        if ekf:
            hf, Ha, Hx, He, rr = ekf_obs(ck, clones[int(job["anchor_rank"])], job["p_w"], job["p_fej"], job["inv_depth"], job["obs_anchor"], z[t], if_fej)
            G[2 * t:2 * t + 2, 7:13] = Ha; G[2 * t:2 * t + 2, 13 + 6 * t:19 + 6 * t] = Hx; G[2 * t:2 * t + 2, c - 1] = hf; Hf[2 * t:2 * t + 2, 0] = hf
        else:
            Hx, He, hf, rr = msckf_obs(ck, job["p_w"], z[t], if_fej)
            G[2 * t:2 * t + 2, 7 + 6 * t:13 + 6 * t] = Hx; Hf[2 * t:2 * t + 2] = hf
        G[2 * t:2 * t + 2, 0:6] = He
        if estimate_td:
            G[2 * t:2 * t + 2, 6] = _v(zv[t])
        r[2 * t:2 * t + 2] = rr
    return G, Hf, r


def column_map(job, ranks, leg_dim):
    M = int(job["n_obs"])
    cols = list(range(15, 22))
    if int(job["type"]) != 0:
        cols += [leg_dim + 6 * int(job["anchor_rank"]) + k for k in range(6)]
    for t in range(M):
        cols += [leg_dim + 6 * int(ranks[t]) + k for k in range(6)]
    if int(job["type"]) != 0:
        cols.append(int(job["fcol"]))
    return np.array(cols, np.int64)


# ---------------------------------------------------------------- long-double linear algebra
def solve_ld(A, B):
    """A X = B by Gaussian elimination with partial pivoting, long double (A square; B vector or matrix)"""
    A = np.array(A, LD); B = np.array(B, LD); vec = B.ndim == 1
    if vec:
        B = B[:, None]
    n = A.shape[0]
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]; B[[k, p]] = B[[p, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= np.outer(f, A[k, k:]); B[k + 1:] -= np.outer(f, B[k])
    X = np.zeros_like(B)
    for k in range(n - 1, -1, -1):
        X[k] = (B[k] - A[k, k + 1:] @ X[k + 1:]) / A[k, k]
    return X[:, 0] if vec else X


def projector(Hf):
    """I - H_f (H_f^T H_f)^-1 H_f^T"""
    return np.eye(Hf.shape[0], dtype=LD) - Hf @ solve_ld(Hf.T @ Hf, Hf.T)


def projected_grams(G, Hf, r):
    """(G'^T G', G'^T r') for the rows projected on null(H_f^T); basis-free"""
    Pi = projector(Hf)
    return G.T @ Pi @ G, G.T @ Pi @ r


def gate_gamma(G, Hf, r, Pcc, sigma2):
    """gamma of the projected rows (Hf = None: the raw rows, EKF_TRACKED).  G: compact rows, Pcc = P[cc][:, cc]"""
    W = G @ np.asarray(Pcc, np.float64).astype(LD) @ G.T + LD(sigma2) * np.eye(G.shape[0], dtype=LD)
    rW = solve_ld(W, r)
    g = r @ rW
    if Hf is not None:
        b = Hf.T @ rW
        g -= b @ solve_ld(Hf.T @ solve_ld(W, Hf), b)
    return g


def null_basis(Hf):
    """an orthonormal basis of null(H_f^T) in float64 (for kappa(S) only)"""
    Q, _ = np.linalg.qr(np.asarray(Hf, np.float64), mode="complete")
    return Q[:, Hf.shape[1]:]


def gate_matrix(G, Hf, Pcc, sigma2):
    """S = G' P G'^T + sigma2 I in float64, for its condition number"""
    G = np.asarray(G, np.float64)
    Gp = G if Hf is None else null_basis(Hf).T @ G
    return Gp @ np.asarray(Pcc, np.float64) @ Gp.T + sigma2 * np.eye(Gp.shape[0])


# ---------------------------------------------------------------- forward-error bounds (derivation: tests/test_gpu_feature_rows.py)
C_GRAM = 2.0
C_GAMMA = 4.0
K_JAC = 16                                   # flops on the longest path of one Jacobian entry (3x3 products of 3x3 products, then dz)


def jac_bound(H, scale=None):
    """entrywise bound on a Jacobian block computed in double: 4 K_JAC u times the largest entry of its row (an entry may be the
    difference of products of that size), or times the given scale (a residual: |z| + |r|)"""
    H = np.asarray(H, np.float64)
    if scale is None:
        scale = np.abs(H).max(axis=-1, keepdims=True) if H.ndim == 2 else np.abs(H).max()
    return 4 * K_JAC * U * scale


def residual_scale(r, z):
    """|r| + |z| per row: the residual z - p_c / p_c[2] is a difference, its rounding error follows |z|"""
    return np.abs(np.asarray(r, np.float64)) + np.abs(np.asarray(z, np.float64)).ravel()


def gram_bound(G, Hf, extra=None):
    """componentwise bound on G'^T G' (and on G'^T r' with extra = residual_scale(r, z)): C_GRAM / 2 (e_i |g_j| + |g_i| e_j), where
    e_j = (m nf + K_JAC) u |g_j| + 4 K_JAC u |rho| bounds the error of the computed column j (Householder: m nf u |g_j|; the
    Jacobian entries: jac_bound, rho = the rows' largest entries) and |g_j| its 2-norm"""
    G = np.asarray(G, np.float64); m = G.shape[0]; nf = 0 if Hf is None else Hf.shape[1]
    n = np.linalg.norm(G, axis=0)
    e = (m * nf + K_JAC) * U * n + 4 * K_JAC * U * np.linalg.norm(np.abs(G).max(axis=1))
    if extra is None:
        return C_GRAM / 2 * (np.outer(e, n) + np.outer(n, e))
    nr = np.linalg.norm(np.asarray(extra, np.float64))
    return C_GRAM / 2 * (e[:, None] * nr + n[:, None] * (m * nf + K_JAC) * U * nr)


def gamma_bound(G, Hf, Pcc, sigma2, gamma, rscale=None):
    """C_GAMMA (k + c) u kappa_2(S) gamma (relative errors of size (k + c) u in S), plus the first-order effect of the residual's
    rounding: 2 sqrt(gamma / lambda_min(S)) |dr'| with |dr'| <= C_GRAM (m nf + K_JAC) u | |r| + |z| | (rscale = residual_scale(r, z))"""
    S = gate_matrix(G, Hf, Pcc, sigma2)
    w = np.linalg.eigvalsh(S)
    kappa = abs(w).max() / abs(w).min()
    g = abs(float(gamma))
    b = C_GAMMA * (S.shape[0] + G.shape[1]) * U * kappa * g
    if rscale is not None:
        m = G.shape[0]; nf = 0 if Hf is None else Hf.shape[1]
        b += 2 * np.sqrt(g / abs(w).min()) * C_GRAM * (m * nf + K_JAC) * U * np.linalg.norm(np.asarray(rscale, np.float64))
    return b


# ---------------------------------------------------------------- scenes
CLONE = np.dtype([("id", np.int64), ("time", np.float64), ("dt", np.float64), ("q", np.float64, 4), ("p", np.float64, 3),
                  ("p_fej", np.float64, 3), ("R_b2c", np.float64, 9), ("t_c_b", np.float64, 3), ("q_cam", np.float64, 4),
                  ("p_cam", np.float64, 3)])


def _rotv(w):
    th = np.linalg.norm(w)
    if th < 1e-15:
        return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _quat(R):
    w = np.sqrt(max(1e-300, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def window(seed, n_clones):
    """a sliding window of n_clones clones on a gentle path (camera z = world z), extrinsics shared"""
    rng = np.random.default_rng(seed)
    R_b2c = _rotv(rng.normal(0, 0.02, 3)) @ np.array([[0, 1.0, 0], [-1, 0, 0], [0, 0, 1]])
    t_c_b = rng.normal(0, 0.05, 3)
    cl = np.zeros(n_clones, CLONE)
    step = 0.4 / max(n_clones, 8) * 8 / 4
    for i in range(n_clones):
        R = _rotv(rng.normal(0, 0.05, 3)); p = np.array([step * i, 0.02 * np.sin(i), 0.01 * i / n_clones]) + rng.normal(0, 0.01, 3)
        cl[i]["id"] = 100 + i; cl[i]["q"] = _quat(R); cl[i]["p"] = p; cl[i]["p_fej"] = p + rng.normal(0, 1e-3, 3)
        cl[i]["R_b2c"] = R_b2c.ravel(); cl[i]["t_c_b"] = t_c_b
        cl[i]["q_cam"] = _quat(R @ R_b2c.T); cl[i]["p_cam"] = p + R @ t_c_b
    return cl


def cam_pose(clone):
    """camera-to-world rotation and position of a clone (the triangulation's view pose)"""
    R = np.asarray(rot(clone["q"]), np.float64) @ np.asarray(clone["R_b2c"]).reshape(3, 3).T
    return R, np.asarray(clone["p"]) + np.asarray(rot(clone["q"]), np.float64) @ np.asarray(clone["t_c_b"])


def project(clone, p_w):
    R, t = cam_pose(clone)
    pc = R.T @ (p_w - t)
    return pc[:2] / pc[2], pc


def landmark(rng, clones, depth=(3.0, 6.0)):
    R, t = cam_pose(clones[0])
    return t + R @ np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.6, 0.6), rng.uniform(*depth)])
