"""Long-double restatement of what lvk_ekf_msckf_point_cov (include/lvk_c.h) defines: for a point p_w with M observations from distinct
clones,
    A = sum_t Hf_t^T Hf_t,   G_t = A^-1 Hf_t^T,   B = sum_t G_t Hc[2t:2t+2, :],   Sigma = sigma2 A^-1 + B P[cc, cc] B^T.

Two routes to the per-observation Jacobians:
  * jacobians_nd(): central differences of a projection function written from the geometry - the camera-frame point after the filter's
    state injection (clone attitude q <- small_angle_quat(d_theta) * q, position p <- p + d_p, extrinsics R_b2c <- R_b2c R(d_theta_e)^T,
    t_c_b <- t_c_b + d_t), then (x / z, y / z).  No derivative is written down on that route.  Under first-estimate Jacobians the lever
    arm of the two rotations is taken at the clone's first-estimate position p_fej, everything else at the current estimate.
  * the analytic route (jacobians_tracked()): the closed-form matrices, carried through a first-order running error analysis of the
    float64 operations the kernel performs (class V below).  tests/test_msckf_point_ref.py holds the two routes to each other.
The GPU tests compare the kernel with the analytic route's long-double value inside the derived bound; the central-difference route
ties that value to the geometry.

The error vector of one observation is ordered as the compact columns: [d_theta_e(3) d_t(3) | td | d_theta(3) d_p(3) of its clone]."""
import numpy as np

from tests.landmark_cov_ref import quat_to_rot, quat_mul, small_angle_quat, skew, random_spd      # noqa: F401  (helpers pinned by test_landmark_cov_ref.py)

LD = np.longdouble
U = LD(2.0) ** -53                # unit roundoff of the kernel's arithmetic
U_LD = LD(np.finfo(LD).eps) / 2   # ... and of this file's
H_STEP = LD(2.0) ** -21           # central-difference step, as landmark_cov_ref.H_STEP
# the analytic B against the central-difference B, relative to |G| |Hc| summed entrywise: truncation h^2 f''' / 6 ~ 4e-14 f''' and
# rounding 2^-64 / h ~ 1e-13 per difference; 1e-10 leaves room for f''' ~ 1e3 (a point 0.5 m from a camera)
TOL_ND = 1e-10


# ------------------------------------------------------------------------------------------------ the problem
def _ld(x):
    return np.asarray(x, np.float64).astype(LD)


def cam_point(clone, p_w, d_x=None, d_e=None, p_ref=None):
    """the point in the camera frame of one clone after the injection of d_x = [d_theta d_p] into the clone and d_e = [d_theta_e d_t]
    into the extrinsics; p_ref: the clone position the world vector is taken from (p, or p_fej for the first-estimate lever arm)"""
    d_x = np.zeros(6, LD) if d_x is None else np.asarray(d_x, LD)
    d_e = np.zeros(6, LD) if d_e is None else np.asarray(d_e, LD)
    q = quat_mul(small_angle_quat(d_x[0:3]), _ld(clone["q"]))
    p = (_ld(clone["p"]) if p_ref is None else np.asarray(p_ref, LD)) + d_x[3:6]
    R_b2c = _ld(clone["R_b2c"]).reshape(3, 3) @ quat_to_rot(small_angle_quat(d_e[0:3])).T
    t_c_b = _ld(clone["t_c_b"]) + d_e[3:6]
    return R_b2c @ (quat_to_rot(q).T @ (np.asarray(p_w, LD) - p) - t_c_b)


def project(p_c):
    return np.array([p_c[0] / p_c[2], p_c[1] / p_c[2]], LD)


def jacobians_nd(clone, p_w, if_fej, h=H_STEP):
    """(Hx 2x6, He 2x6, Hf 2x3) by central differences: D project at the current camera-frame point, times D cam_point with the lever arm
    at p_fej when if_fej"""
    p_w = _ld(p_w)
    pc0 = cam_point(clone, p_w)
    Dpi = np.zeros((2, 3), LD)
    for k in range(3):
        d = np.zeros(3, LD); d[k] = h
        Dpi[:, k] = (project(pc0 + d) - project(pc0 - d)) / (2 * h)
    ref = _ld(clone["p_fej"]) if if_fej else _ld(clone["p"])
    Dx = np.zeros((3, 6), LD); De = np.zeros((3, 6), LD); Df = np.zeros((3, 3), LD)
    for k in range(6):
        d = np.zeros(6, LD); d[k] = h
        Dx[:, k] = (cam_point(clone, p_w, d_x=d, p_ref=ref) - cam_point(clone, p_w, d_x=-d, p_ref=ref)) / (2 * h)
        De[:, k] = (cam_point(clone, p_w, d_e=d, p_ref=ref) - cam_point(clone, p_w, d_e=-d, p_ref=ref)) / (2 * h)
    for k in range(3):
        d = np.zeros(3, LD); d[k] = h
        Df[:, k] = (cam_point(clone, p_w + d, p_ref=ref) - cam_point(clone, p_w - d, p_ref=ref)) / (2 * h)
    return Dpi @ Dx, Dpi @ De, Dpi @ Df


def columns(ranks, leg_dim):
    """the column map cc of a job: 15..21, then leg_dim + 6 rank_t + j"""
    return np.concatenate([np.arange(15, 22)] + [leg_dim + 6 * int(r) + np.arange(6) for r in ranks])


def ldl3(A):
    """unpivoted LDL^T of a 3 x 3 matrix -> (L, d); the pivots are d"""
    L = np.eye(3, dtype=A.dtype); d = np.zeros(3, A.dtype)
    d[0] = A[0, 0]
    L[1, 0] = A[1, 0] / d[0]; L[2, 0] = A[2, 0] / d[0]
    d[1] = A[1, 1] - L[1, 0] * L[1, 0] * d[0]
    L[2, 1] = (A[2, 1] - L[2, 0] * L[1, 0] * d[0]) / d[1]
    d[2] = A[2, 2] - L[2, 0] * L[2, 0] * d[0] - L[2, 1] * L[2, 1] * d[1]
    return L, d


def inv3(A):
    L, d = ldl3(A)
    Li = np.eye(3, dtype=A.dtype)
    Li[1, 0] = -L[1, 0]; Li[2, 1] = -L[2, 1]; Li[2, 0] = L[1, 0] * L[2, 1] - L[2, 0]
    return Li.T @ np.diag(1 / d) @ Li


def assemble(H, zv, estimate_td, Pcc, sigma2):
    """the definition, plainly, from per-observation (Hx, He, Hf) triples -> (Sigma, B, Ainv, A)"""
    M = len(H); c = 7 + 6 * M
    A = np.zeros((3, 3), LD)
    for _, _, Hf in H:
        A = A + Hf.T @ Hf
    Ainv = inv3(A)
    B = np.zeros((3, c), LD)
    for t, (Hx, He, Hf) in enumerate(H):
        G = Ainv @ Hf.T
        B[:, 0:6] += G @ He
        if estimate_td:
            B[:, 6] += G @ _ld(zv[t])
        B[:, 7 + 6 * t:13 + 6 * t] = G @ Hx
    return LD(sigma2) * Ainv + B @ Pcc @ B.T, B, Ainv, A


def sigma_nd(prob, P):
    """Sigma by the central-difference route -> (Sigma, B, Ainv, A)"""
    H = [jacobians_nd(prob["clones"][r], prob["p_w"], prob["if_fej"]) for r in prob["ranks"]]
    cc = columns(prob["ranks"], prob["leg_dim"])
    return assemble(H, prob["zv"], prob["estimate_td"], np.asarray(P, np.float64)[np.ix_(cc, cc)].astype(LD), prob["sigma2"])


# ------------------------------------------------------------------------------------------------ running error analysis
class V:
    """a long-double value v with an entrywise first-order bound e on the error of its float64 computation.  Every operation adds
    the rounding of its own result (u |result|, or gamma_k |a| |b| for a length-k inner product) to what its operands carry."""
    def __init__(self, v, e=None):
        self.v = np.asarray(v, LD); self.e = np.zeros(self.v.shape, LD) if e is None else np.asarray(e, LD)

    def __add__(self, o):
        o = _V(o); v = self.v + o.v
        return V(v, self.e + o.e + U * np.abs(v))

    def __sub__(self, o):
        o = _V(o); v = self.v - o.v
        return V(v, self.e + o.e + U * np.abs(v))

    def __mul__(self, o):
        o = _V(o); v = self.v * o.v
        return V(v, np.abs(self.v) * o.e + self.e * np.abs(o.v) + U * np.abs(v))

    def __truediv__(self, o):
        o = _V(o); v = self.v / o.v
        return V(v, self.e / np.abs(o.v) + np.abs(v) * o.e / np.abs(o.v) + U * np.abs(v))

    def __neg__(self):
        return V(-self.v, self.e)

    def __getitem__(self, k):
        return V(self.v[k], self.e[k])

    @property
    def T(self):
        return V(self.v.T, self.e.T)


def _V(x):
    return x if isinstance(x, V) else V(x)


def mm(a, b):
    """matrix product, each entry one inner product of length k summed in order: gamma_k |a| |b| on top of the operands' errors"""
    a = _V(a); b = _V(b); k = a.v.shape[-1]
    return V(a.v @ b.v, np.abs(a.v) @ b.e + a.e @ np.abs(b.v) + k * U * (np.abs(a.v) @ np.abs(b.v)))


def stack(rows):
    """a matrix (list of lists) or vector (list) of scalar V / numbers -> V"""
    if isinstance(rows[0], (list, tuple)):
        return V([[_V(x).v for x in r] for r in rows], [[_V(x).e for x in r] for r in rows])
    return V([_V(x).v for x in rows], [_V(x).e for x in rows])


def hcat(a, b):
    return V(np.concatenate([a.v, b.v], axis=1), np.concatenate([a.e, b.e], axis=1))


def skew_v(w):
    """[w]x: no arithmetic, the entries and their errors move"""
    return V(skew(w.v), np.abs(skew(w.e)))


def quat_to_rot_v(q):
    x, y, z, w = (V(c) for c in _ld(q))
    tx, ty, tz = x * 2, y * 2, z * 2              # (exact in binary; counted anyway)
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = V(LD(1))
    return stack([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]])


def jacobians_tracked(clone, p_w, if_fej):
    """(Hx, He, Hf) as V: the closed forms of the measurement Jacobian of a point seen from one clone, with the error of the kernel's
    float64 evaluation of them.  With R = R(q) (body to world), R_w2c = R_b2c R^T, p_c = R_w2c (p_w - p - R t_c_b), l = p_w - p_ref:
      D project = [1/z 0 -x/z^2; 0 1/z -y/z^2],  d p_c = R_w2c [l]x d_theta - R_w2c d_p + (R_w2c [l]x R - R_b2c [t_c_b]x) d_theta_e - R_b2c d_t,
      d p_c / d p_w = R_w2c."""
    R_b2c = V(_ld(clone["R_b2c"]).reshape(3, 3)); t_c_b = V(_ld(clone["t_c_b"])); p = V(_ld(clone["p"])); pw = V(_ld(p_w))
    R_b2w = quat_to_rot_v(clone["q"])
    R_w2c = mm(R_b2c, R_b2w.T)
    p_c = mm(R_w2c, pw - (p + mm(R_b2w, t_c_b)))
    lever = pw - V(_ld(clone["p_fej"])) if if_fej else pw - p
    x, y, z = p_c[0], p_c[1], p_c[2]
    one = V(LD(1)); zero = V(LD(0))
    dz = stack([[one / z, zero, -(x / (z * z))], [zero, one / z, -(y / (z * z))]])
    A_ = mm(R_w2c, skew_v(lever))
    dxb = hcat(A_, -R_w2c)
    dxe = hcat(mm(A_, R_b2w) - mm(R_b2c, skew_v(t_c_b)), -R_b2c)
    return mm(dz, dxb), mm(dz, dxe), mm(dz, R_w2c)


def sigma_tracked(prob, P):
    """-> (Sigma, err, Bnd, cond): the long-double Sigma of the analytic route, the derived componentwise bound on the float64 kernel's
    error against it, the entrywise scale Bnd = sigma2 |A^-1| + |B| |P_cc| |B|^T and cond_2(A).

    The bound is first order in u = 2^-53 and follows the kernel operation by operation (class V): the Jacobians; A, a running sum
    over the observations; the 3 x 3 solves, by the perturbation result for an LDL^T solve,
        |dx| <= |A^-1| ((dA + gamma_10 |L| |D| |L^T|) |x| + db)
    (dA, db: what A and the right-hand side carry; gamma_10: factorisation plus two substitutions at n = 3) - this is the cond(A) term;
    B from 2-term products and a running sum over the observations for its first seven columns; T = B P_cc and T B^T as inner
    products of length c (gamma_c |.| |.|); the final scale by sigma2 and sum.  On top: this file's own rounding, u_ld / u of the same
    expression.  Nothing in it is fitted to a result."""
    ranks = prob["ranks"]; M = len(ranks); c = 7 + 6 * M
    cc = columns(ranks, prob["leg_dim"])
    Pcc = np.asarray(P, np.float64)[np.ix_(cc, cc)].astype(LD)
    H = [jacobians_tracked(prob["clones"][r], prob["p_w"], prob["if_fej"]) for r in ranks]
    A = V(np.zeros((3, 3), LD))
    for _, _, Hf in H:
        A = A + mm(Hf.T, Hf)
    L, d = ldl3(A.v)
    Ainv = inv3(A.v)
    dA = A.e + 10 * U * (np.abs(L) @ np.diag(np.abs(d)) @ np.abs(L).T)
    aAinv = np.abs(Ainv)
    Ainv_v = V(Ainv, aAinv @ dA @ aAinv)
    Bv = np.zeros((3, c), LD); Be = np.zeros((3, c), LD)
    head = V(np.zeros((3, 7), LD))
    for t, (Hx, He, Hf) in enumerate(H):
        Gv = Ainv @ Hf.v.T
        G = V(Gv, aAinv @ (dA @ np.abs(Gv) + Hf.e.T))
        zv = _ld(prob["zv"][t]).reshape(2, 1) if prob["estimate_td"] else np.zeros((2, 1), LD)
        head = head + mm(G, hcat(He, V(zv)))
        blk = mm(G, Hx)
        Bv[:, 7 + 6 * t:13 + 6 * t] = blk.v; Be[:, 7 + 6 * t:13 + 6 * t] = blk.e
    Bv[:, :7] = head.v; Be[:, :7] = head.e
    B = V(Bv, Be)
    S = V(LD(prob["sigma2"])) * Ainv_v + mm(mm(B, V(Pcc)), B.T)
    err = np.triu(S.e) + np.triu(S.e, 1).T                      # the kernel computes the upper triangle and copies it
    Bnd = LD(prob["sigma2"]) * aAinv + np.abs(Bv) @ np.abs(Pcc) @ np.abs(Bv).T
    err = err * (1 + U_LD / U) + U_LD * Bnd * c
    ev = np.linalg.eigvalsh(A.v.astype(np.float64))
    return S.v, err, Bnd, float(ev[-1] / ev[0])


def B_tracked(prob):
    """the analytic route's B (3 x c), for the comparison with the central-difference route"""
    H = [tuple(m.v for m in jacobians_tracked(prob["clones"][r], prob["p_w"], prob["if_fej"])) for r in prob["ranks"]]
    c = 7 + 6 * len(H)
    return assemble(H, prob["zv"], prob["estimate_td"], np.zeros((c, c), LD), 0.0)[1]


# ------------------------------------------------------------------------------------------------ test problems
def make_clones(rng, n_clones, step=0.15):
    """a window of clones on a gently curving track: ~step metres apart along x, attitudes within 0.15 rad of a common heading, a camera
    rotated and offset from the body like a real rig and looking along world +z; p_fej a centimetre off p"""
    from larvio_amd.larvio import CLONE
    cl = np.zeros(n_clones, CLONE)
    qe = np.array([0.02, -0.03, 0.7071, 0.7071]); qe /= np.linalg.norm(qe)
    R_b2c = np.asarray(quat_to_rot(qe), np.float64)
    for i in range(n_clones):
        a = rng.uniform(-0.15, 0.15, 3)
        q = np.array([a[0] / 2, a[1] / 2, a[2] / 2, 1.0]); q /= np.linalg.norm(q)
        cl[i]["id"] = i; cl[i]["q"] = q
        cl[i]["p"] = [step * i + rng.uniform(-0.02, 0.02), 0.08 * np.sin(0.3 * i) + rng.uniform(-0.02, 0.02), 0.05 * np.cos(0.2 * i)]
        cl[i]["p_fej"] = cl[i]["p"] + rng.normal(0, 0.01, 3)
        cl[i]["R_b2c"] = R_b2c.reshape(9); cl[i]["t_c_b"] = [0.05, -0.02, 0.01]
    return cl


def make_problem(rng, clones, ranks, leg_dim=22, if_fej=False, estimate_td=False, sigma2=6.4e-5, noise=1e-3, p_w=None):
    """one point seen from clones[ranks] (in that order): p_w 3 - 7 m in front of the middle of the track unless given, observations =
    its projections + noise, zv = image velocities of a few tenths per second"""
    ranks = [int(r) for r in ranks]
    if p_w is None:
        mid = np.mean([clones[r]["p"] for r in ranks], axis=0)
        p_w = mid + np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(3.0, 7.0)])
    z = np.array([np.asarray(project(cam_point(clones[r], p_w)), np.float64) for r in ranks]) + rng.normal(0, noise, (len(ranks), 2))
    zv = rng.uniform(-0.3, 0.3, (len(ranks), 2))
    return dict(clones=clones, ranks=ranks, p_w=np.asarray(p_w, np.float64), z=z, zv=zv, leg_dim=leg_dim, if_fej=bool(if_fej), estimate_td=bool(estimate_td),
                sigma2=float(sigma2))


def degenerate_problem(n_clones_needed=4, leg_dim=22):
    """all cameras at one position with one attitude, the point on the optical axis: every Hf_t is [1/z 0 0; 0 1/z 0] exactly, A =
    diag(M/z^2, M/z^2, 0) exactly, and the third pivot of the LDL^T is exactly 0"""
    from larvio_amd.larvio import CLONE
    cl = np.zeros(n_clones_needed, CLONE)
    for i in range(n_clones_needed):
        cl[i]["id"] = i; cl[i]["q"] = [0, 0, 0, 1]; cl[i]["R_b2c"] = np.eye(3).reshape(9)
    ranks = list(range(n_clones_needed))
    return dict(clones=cl, ranks=ranks, p_w=np.array([0.0, 0.0, 4.0]), z=np.zeros((len(ranks), 2)), zv=np.zeros((len(ranks), 2)), leg_dim=leg_dim, if_fej=False,
                estimate_td=False, sigma2=6.4e-5)


def correlated_position_cov(n, ranks, leg_dim, s2):
    """P with the position blocks of the observing clones at s2 I, fully correlated with one another, everything else zero: every
    observing clone's position error is the same vector ~ N(0, s2 I)"""
    P = np.zeros((n, n))
    cols = [leg_dim + 6 * int(r) + 3 for r in ranks]
    for a in cols:
        for b in cols:
            P[a:a + 3, b:b + 3] = s2 * np.eye(3)
    return P


# ------------------------------------------------------------------------------------------------ the launches of the GPU stage tests
N_MAX = 433
PAD = 5


def pack(probs):
    """the stage entry's arrays for a list of problems of one launch -> (jobs, clone_rank, obs, obs_vel)"""
    from larvio_amd.ops import MSCKF_POINT_JOB
    jobs = np.zeros(len(probs), MSCKF_POINT_JOB); rk = []; z = []; zv = []
    for k, pr in enumerate(probs):
        jobs[k]["n_obs"] = len(pr["ranks"]); jobs[k]["obs_off"] = len(rk); jobs[k]["p_w"] = pr["p_w"]
        rk += pr["ranks"]; z += list(pr["z"]); zv += list(pr["zv"])
    return jobs, np.array(rk, np.int32), np.array(z, np.float64).reshape(-1, 2), np.array(zv, np.float64).reshape(-1, 2)


def buffer(P, n, ldp):
    """P in a row-major buffer of leading dimension ldp, NaN in the padding (never read)"""
    b = np.full((n, ldp), np.nan); b[:, :n] = P
    return b


_LAUNCHES = None


def stage_launches():
    """Every launch the GPU stage tests make against the restatement, built once: M = 2, 3, 31, 32, 33, 62, 63, 64 (one launch each,
    the eight combinations of leg_dim 22 / 46, estimate_td, if_fej spread over them; n alternating between the smallest that holds
    the job, leg_dim + 6 M, and 433; ldp alternating between n and n + PAD; ranks alternating between descending and scattered;
    1 or 7 jobs), and one launch of 300 short jobs.  -> list of dict(name, clones, probs, P, n, ldp, leg_dim, if_fej, estimate_td, sigma2)"""
    global _LAUNCHES
    if _LAUNCHES is not None:
        return _LAUNCHES
    import itertools
    out = []
    flags = list(itertools.product((22, 46), (0, 1), (0, 1)))
    for k, M in enumerate((2, 3, 31, 32, 33, 62, 63, 64)):
        rng = np.random.default_rng([20261018, M])
        leg, td, fej = flags[k]
        small = k % 2 == 0
        n = leg + 6 * M if small else N_MAX
        n_clones = (n - leg) // 6
        clones = make_clones(rng, n_clones)
        n_jobs = 1 if M == 2 else 7 if M in (3, 33) else 2
        probs = []
        for j in range(n_jobs):
            pick = np.sort(rng.choice(n_clones, M, replace=False))[::-1]
            if (k + j) % 2:
                pick = rng.permutation(pick)
            probs.append(make_problem(rng, clones, pick, leg_dim=leg, if_fej=fej, estimate_td=td))
        out.append(dict(name="M%d" % M, clones=clones, probs=probs, P=random_spd(rng, n), n=n, ldp=n if k % 4 < 2 else n + PAD, leg_dim=leg, if_fej=fej,
                        estimate_td=td, sigma2=probs[0]["sigma2"]))
    rng = np.random.default_rng([20261018, 300])
    clones = make_clones(rng, 12); n = 22 + 6 * 12
    probs = [make_problem(rng, clones, rng.permutation(rng.choice(12, int(rng.integers(2, 5)), replace=False)), if_fej=1, estimate_td=1) for _ in range(300)]
    out.append(dict(name="300 jobs", clones=clones, probs=probs, P=random_spd(rng, n), n=n, ldp=n + PAD, leg_dim=22, if_fej=1, estimate_td=1, sigma2=probs[0]["sigma2"]))
    _LAUNCHES = out
    return out
