"""The factor-and-solve of the default update route (k_chol_fused + launch_chol_solve, larvio_amd/csrc/be_linalg.hip; stage entry
lvk_chol_solve) restated in numpy.longdouble:  S = L L^T,  W = L^-1 B,  G = W^T W,  X = S^-1 B = L^-T W  - and componentwise bounds
on what the FP64 kernel may return for W, for G and for the blocks of L it stores (bounds), derived for the algorithm the kernel
runs, not measured on it.  Long double (x87 extended, u = 2^-64 on the machines the suite runs on) stands for the exact answer.
Also here: the filter-like problems of the stage tests (problem / find_problem / the case lists), so that the CPU self-test
(tests/test_chol_ref.py) and the GPU tests (tests/test_gpu_chol_stages.py) see the same ones, and a plain FP64 emulation of the blocked
algorithm (emulate) that the self-test holds against the bound, with and without planted faults.

The algorithm.  Rows come in panels of NB = 32 inside super-blocks of MB = 160; panel j covers columns c_j .. c_j + k_j - 1.
  diagonal block (chol32_inv_mfma):  A_jj = L_jj L_jj^T unblocked, 1 / sqrt(pivot) from v_rsq_f64 and two coupled Goldschmidt steps, the
      column scaled by a product;  Y_j = L_jj^-1 EXPLICITLY: Y00, Y11 (16 x 16 halves) by column-oriented substitution with the same
      reciprocal roots, Y10 = -Y11 (L10 Y00) by two 16-term products.  L_jj itself never leaves the registers.
  below it:  L_ij = A_ij Y_j^T (32-term products);  trailing blocks A_il -= L_ij L_lj^T (right-looking inside a super-block).
  solve:     W_j = Y_j t_j,  t_j = B_j - sum_{q<j} L_jq W_q.
  recursion: for rows beyond a super-block, L21^T = L11^-1 S12 by the same solve (second right-hand side), then the GEMMs
      S22 -= L21 L21^T and B2 -= L21 W1 (k_dgemm_sk: split-K, fixed order), and on with (S22, B2).

The derivation (first order in u = 2^-53; sources: Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed. - (3.5) and section
4.2 for sums and dot products in ANY order, Theorem 8.5 for substitution, Theorem 10.3 for Cholesky; Chang, Paige, Stewart, New
perturbation analyses for the Cholesky factorization, IMA J. Numer. Anal. 16 (1996), for dL = L Phi(L^-1 dS L^-T)).
 (a) Every entry of a block as it stands when its panel is reached, A^_ij = S_ij - sum_{q<j} L^_iq L^_jq^T + d_ij (hats: computed), is a
     sum of c_j + 1 terms, c_j of them products, whatever the grouping (32-term matrix-core chains, the GEMM's four partial sums, one
     subtraction per panel or per super-block):   |d_ij| <= gamma_{c_j+2} (|S_ij| + sum_{q<j} |L_iq||L_jq|^T).    Likewise
     t^_j = B_j - sum_{q<j} L^_jq W^_q + e_j,  |e_j| <= gamma_{c_j+2} (|B_j| + sum_{q<j} |L_jq||W_q|).
 (b) The reciprocal root: the seed's error is squared twice (2^-20 -> ~1e-24), what is left is the rounding of the last coupled step,
     |rinv sqrt(x) - 1| <= 4u; a column entry is one more product.  With a division replaced by that product Theorem 10.3 gives, for
     the factor L~_jj the kernel holds in registers,  L~_jj L~_jj^T = A^_jj + D_j,  |D_j| <= gamma_{k_j+6} |L_jj||L_jj|^T.
     DEFINE L^_jj := L~_jj.  Then L^ (with the computed blocks below) is the exact Cholesky factor of S + dS.
 (c) Y^_j against L^_jj^-1 (Theorem 8.5 per column, with (b) for the scaling; the halves have at most 16 rows):
       EY00 = gamma_22 |Y00||L00||Y00|,  EY11 = gamma_22 |Y11||L11||Y11|,
       EY10 = 2 gamma_16 |Y11||L10||Y00| + EY11 |L10||Y00| + |Y11||L10| EY00          (two products, and the errors of their operands).
 (d) L^_ij = fl(A^_ij Y^_j^T), i > j:  L^_ij L^_jj^T = A^_ij + A^_ij (Y^_j - L^_jj^-1)^T L^_jj^T + (product rounding) L^_jj^T, so with (a)
       |dS_ij| <= gamma_{c_j+2} (|S_ij| + sum_{q<j} |L_iq||L_jq|^T) + |A_ij| (EY_j^T + gamma_32 |Y_j|^T) |L_jj|^T,   A_ij = L_ij L_jj^T,
       |dS_jj| <= gamma_{c_j+2} (...) + gamma_{k_j+6} |L_jj||L_jj|^T.          =: ES  (symmetric).
     The same holds, transposed, for L21^T = fl(Y^_j t^) of the recursion.  This is where |L_jj^-1||L_jj| enters: a substitution would
     not have it.
 (e) The solve's residual R = L^ W^ - B:  L^_jj W^_j = L^_jj (Y^_j t^_j + product rounding), hence
       |R_j| <= gamma_{c_j+2} (|B_j| + sum_{q<j} |L_jq||W_q|) + |L_jj| (EY_j + gamma_32 |Y_j|) |t_j|,   t_j = L_jj W_j.      =: RB
 (f) W^ = L^^-1 (B + R) and L^ L^^T = S + dS, so G^ = W^^T W^ = (B + R)^T (S + dS)^-1 (B + R) and, to first order,
       G^ - G = R^T X + X^T R - X^T dS X :      |G^ - G| <= |X|^T ES |X| + RB^T |X| + |X|^T RB          (no |S^-1| anywhere),
       L^ - L = L Phi(L^-1 dS L^-T)       :      |L^ - L| <= |L| Phi(|L^-1| ES |L^-T|)  =: EL       (Phi: lower triangle, diagonal halved),
       W^ - W = L^-1 (R - (L^ - L) W)     :      |W^ - W| <= |L^-1| (RB + EL |W|).
 The neglected terms multiply a bound by 1 / (1 - eps) with eps of the size of max(|L^-1| ES |L^-T|) and of bound / solution; every bound
 is DOUBLED, which covers eps <= 1/2, and the tests assert eps-like quantities below 0.1 (bounds(...)["eps"] and the 0.1 side
 condition).  No constant here was measured or fitted: all are counts of rounding operations.  The bound matrices themselves are
 evaluated in FP64 (their own relative error, ~1e-13, is immaterial)."""
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
NB, MB = 32, 160
SIGMA = 0.008


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def panels(m):
    """[(c0, c1)]: the 32-row panels; 160 is a multiple of 32, so they are the same inside every super-block"""
    return [(c, min(c + NB, m)) for c in range(0, m, NB)]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def cholesky(S):
    """long-double L (lower) with L L^T = the symmetric matrix that S's lower triangle stands for; raises on a non-positive pivot"""
    A = np.tril(np.asarray(S, LD)); A = A + np.tril(A, -1).T
    m = A.shape[0]
    L = np.zeros((m, m), LD)
    for k in range(m):
        if not A[k, k] > 0:
            raise ValueError(f"pivot {k} is not positive")
        d = np.sqrt(A[k, k])
        L[k:, k] = A[k:, k] / d
        A[k + 1:, k + 1:] -= np.outer(L[k + 1:, k], L[k + 1:, k])
    return L


def forward(L, B):
    W = np.array(B, LD)
    for i in range(L.shape[0]):
        W[i] = (W[i] - L[i, :i] @ W[:i]) / L[i, i]
    return W


def backward(L, W):
    X = np.array(W, LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def reference(S, B):
    L = cholesky(S)
    W = forward(L, B)
    return dict(L=L, W=W, G=W.T @ W, X=backward(L, W))


def stored_mask(m):
    """True where lvk_chol_solve leaves a defined entry of L: below the diagonal 32 x 32 blocks (inside a super-block at its own place,
    across super-blocks transposed in S12 - extract_L undoes that)"""
    r = np.arange(m)[:, None]; c = np.arange(m)[None, :]
    return (r // NB) > (c // NB)


def extract_L(Sout, m):
    """the stored entries of L from the S buffer after the call (zero elsewhere)"""
    Sout = np.asarray(Sout)[:m, :m]
    r = np.arange(m)[:, None]; c = np.arange(m)[None, :]
    same = (r // MB) == (c // MB)
    return np.where(stored_mask(m), np.where(same, Sout, Sout.T), 0.0)


# ---------------------------------------------------------------------------------------------------------------- the bounds
def _ey(Ljj):
    """(c): bound on Y^_j - L^_jj^-1, and |Y_j|"""
    k = Ljj.shape[0]; h = min(16, k)
    aL = np.abs(Ljj); aY = np.abs(np.linalg.inv(Ljj))
    EY = np.zeros((k, k))
    EY[:h, :h] = gamma(22) * (aY[:h, :h] @ aL[:h, :h] @ aY[:h, :h])
    if k > h:
        EY[h:, h:] = gamma(22) * (aY[h:, h:] @ aL[h:, h:] @ aY[h:, h:])
        LY = aL[h:, :h] @ aY[:h, :h]
        EY[h:, :h] = 2 * gamma(16) * (aY[h:, h:] @ LY) + EY[h:, h:] @ LY + aY[h:, h:] @ aL[h:, :h] @ EY[:h, :h]
    return EY, aY


def bounds(S, B, ref):
    """-> dict(W, G, L: componentwise bounds on |computed - exact| (FP64 arrays; L's holds on stored_mask), eps: max |L^-1| ES |L^-T|)"""
    S = np.asarray(S, np.float64); B = np.asarray(B, np.float64)
    m = S.shape[0]
    L = np.asarray(ref["L"], np.float64); aL = np.abs(L)
    aW = np.abs(np.asarray(ref["W"], np.float64)); aX = np.abs(np.asarray(ref["X"], np.float64))
    aS = np.abs(np.tril(S) + np.tril(S, -1).T); aB = np.abs(B)
    ES = np.zeros((m, m)); RB = np.zeros_like(aB)
    for c0, c1 in panels(m):
        Ljj = L[c0:c1, c0:c1]
        EY, aY = _ey(Ljj)
        g = gamma(c0 + 2)
        ES[c0:, c0:c1] = g * (aS[c0:, c0:c1] + aL[c0:, :c0] @ aL[c0:c1, :c0].T)
        ES[c0:c1, c0:c1] += gamma(c1 - c0 + 6) * (aL[c0:c1, c0:c1] @ aL[c0:c1, c0:c1].T)
        if c1 < m:
            Aij = np.abs(np.asarray(ref["L"][c1:, c0:c1] @ ref["L"][c0:c1, c0:c1].T, np.float64))
            ES[c1:, c0:c1] += Aij @ ((EY.T + gamma(32) * aY.T) @ aL[c0:c1, c0:c1].T)
        t = np.abs(np.asarray(ref["L"][c0:c1, c0:c1] @ ref["W"][c0:c1], np.float64))
        RB[c0:c1] = g * (aB[c0:c1] + aL[c0:c1, :c0] @ aW[:c0]) + aL[c0:c1, c0:c1] @ ((EY + gamma(32) * aY) @ t)
    ES = np.tril(ES) + np.tril(ES, -1).T
    Linv = np.abs(np.linalg.inv(L))
    T = Linv @ ES @ Linv.T
    EL = aL @ (np.tril(T, -1) + 0.5 * np.diag(np.diag(T)))
    bW = Linv @ (RB + EL @ aW)
    bG = aX.T @ ES @ aX + RB.T @ aX + aX.T @ RB
    return dict(W=2 * bW, G=2 * bG, L=2 * EL, eps=float(T.max()))


def ratios(Wc, Lc, ref, bnd):
    """worst |error| / bound of W, of G = W^T W (formed in long double from the computed W: its own rounding, m 2^-63 |W|^T|W|, is added
    to the bound) and of the stored blocks of L.  Lc: extract_L of the S buffer, or None."""
    def worst(e, b):
        e = np.asarray(e, np.float64)
        return float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1), np.where(e > 0, np.inf, 0)))) if e.size else 0.0
    Wc = np.asarray(Wc, LD)
    m = Wc.shape[0]
    rW = worst(np.abs(Wc - ref["W"]), bnd["W"])
    aW = np.abs(np.asarray(ref["W"], np.float64))
    rG = worst(np.abs(Wc.T @ Wc - ref["G"]), bnd["G"] + m * 2.0 ** -63 * (aW.T @ aW))
    rL = 0.0
    if Lc is not None:
        mask = stored_mask(m)
        rL = worst(np.abs(np.asarray(Lc, LD) - ref["L"])[mask], bnd["L"][mask])
    return rW, rG, rL


def side_condition(ref, bnd):
    """the first-order analysis stands (see the module docstring): a property of the problem and the restatement alone"""
    m = ref["L"].shape[0]
    mask = stored_mask(m)
    ok = bnd["eps"] < 0.1 and float(bnd["W"].max()) < 0.1 * float(np.abs(ref["W"]).max()) and float(bnd["G"].max()) < 0.1 * float(np.abs(ref["G"]).max())
    if mask.any():
        ok = ok and float(bnd["L"][mask].max()) < 0.1 * float(np.abs(ref["L"]).max())
    return bool(ok)


# ---------------------------------------------------------------------------------------------------------------- the problems
def problem(m, nbcols, seed):
    """Filter-like: P = D C D (C a well-conditioned correlation matrix, D over 1e-4 .. 1: variances over 1e-8 .. 1), H with two to four
    6-column blocks per row, S = H P H^T + sigma^2 I (exactly symmetric), B = the first nbcols - 1 columns of H P and the residual r.
    -> S (m x m), B (m x nbcols), FP64"""
    rng = np.random.default_rng(seed)
    N = 6 * math.ceil(max(nbcols - 1, 42) / 6)
    Z = rng.normal(0, 1, (N, N)); Cm = Z @ Z.T / N + 2 * np.eye(N)
    d = np.sqrt(np.diag(Cm)); Cm = Cm / np.outer(d, d)
    D = 10.0 ** rng.uniform(-4, 0, N); D[0] = 1e-4; D[1] = 1.0
    P = Cm * np.outer(D, D)
    H = np.zeros((m, N))
    for i in range(m):
        for b in rng.choice(N // 6, size=int(rng.integers(2, 5)), replace=False):
            H[i, 6 * b:6 * b + 6] = rng.normal(0, 1, 6)
    r = rng.normal(0, 0.01, m)
    HP = H @ P
    S = HP @ H.T + SIGMA ** 2 * np.eye(m)
    S = np.tril(S) + np.tril(S, -1).T
    B = np.concatenate([HP[:, :nbcols - 1], r[:, None]], axis=1)
    return S, B


@functools.lru_cache(maxsize=None)
def find_problem(m, nbcols):
    """the first seed from 1000 m + nbcols on whose problem meets the side condition -> (S, B, ref, bounds); cached, never modified"""
    for seed in range(1000 * m + nbcols, 1000 * m + nbcols + 50):
        S, B = problem(m, nbcols, seed)
        ref = reference(S, B)
        bnd = bounds(S, B, ref)
        if side_condition(ref, bnd):
            for a in (S, B):
                a.setflags(write=False)
            return S, B, ref, bnd
    raise AssertionError(f"no seed meets the side condition for m {m} nbcols {nbcols}")


PANEL_CASES = [(m, 33) for m in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 159, 160)]
GRID_CASES = [(65, nb) for nb in (1, 15, 16, 17, 48, 49, 64, 65, 129)]
RECURSION_CASES = [(m, 33) for m in (161, 175, 176, 177, 192, 193, 223, 224, 225, 320, 321, 481)]
ALL_CASES = PANEL_CASES + [c for c in GRID_CASES if c not in PANEL_CASES] + RECURSION_CASES
STRIDED_CASES = [(17, 33), (65, 64), (65, 129), (160, 33), (177, 33), (321, 33)]
REPORT_M, REPORT_NB, REPORT_BAD = 200, 33, (0, 31, 32, 159, 160, 199)


def indefinite_problem(bad):
    """m = 200: row and column `bad` of S are zero except S[bad][bad] = sigma^2 - 1 (a direction of variance -1 that this row alone sees)"""
    S, B = problem(REPORT_M, REPORT_NB, 77)
    S[bad, :] = 0.0; S[:, bad] = 0.0; S[bad, bad] = SIGMA ** 2 - 1.0
    return S, B


# ---------------------------------------------------------------------------------------------------------------- FP64 emulation
def _chol32_inv(D):
    k = D.shape[0]; A = D.copy(); L = np.zeros((k, k)); rinv = np.zeros(k)
    for j in range(k):
        rinv[j] = 1.0 / np.sqrt(A[j, j])
        L[j:, j] = A[j:, j] * rinv[j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])

    def sub(Lh, rh):
        Y = np.eye(Lh.shape[0])
        for j in range(Lh.shape[0]):
            Y[j] *= rh[j]
            Y[j + 1:] -= np.outer(Lh[j + 1:, j], Y[j])
        return Y
    h = min(16, k)
    Y = np.zeros((k, k))
    Y[:h, :h] = sub(L[:h, :h], rinv[:h])
    if k > h:
        Y[h:, h:] = sub(L[h:, h:], rinv[h:])
        Y[h:, :h] = -(Y[h:, h:] @ (L[h:, :h] @ Y[:h, :h]))
    return Y


FAULTS = ("drop_chunk", "y_f32", "w_tile", "swap")


def emulate(S, B, fault=None):
    """The blocked algorithm in plain numpy FP64 -> (S buffer, W) as lvk_chol_solve leaves them (extract_L applies).  fault: one of
    FAULTS, planted in the first super-block - a trailing update without its k = 16..31 chunk; Y of the first panel rounded to float32; the
    second 16-column tile of W's first 16 rows taken from the first column group; the leading 16 x 16 tile of W transposed."""
    S = np.array(S, np.float64); W = np.array(B, np.float64)
    m, nb = W.shape
    for off in range(0, m, MB):
        mb = min(MB, m - off); end = off + mb
        pan = [(off + a, off + b) for a, b in panels(mb)]
        Ys = []
        for p, (c0, c1) in enumerate(pan):
            Y = _chol32_inv(S[c0:c1, c0:c1])
            if fault == "y_f32" and off == 0 and p == 0:
                Y = Y.astype(np.float32).astype(np.float64)
            Ys.append(Y)
            S[c1:end, c0:c1] = S[c1:end, c0:c1] @ Y.T
            Lp = S[c1:end, c0:c1]
            upd = Lp @ Lp.T
            if fault == "drop_chunk" and off == 0 and p == 0 and c1 < end:
                a = min(c1 + 16, end) - c1
                upd[:a, :a] = Lp[:a, :16] @ Lp[:a, :16].T
            S[c1:end, c1:end] -= upd
        for R in (W, S[:, end:]):            # the right-hand side, then S12 (second right-hand side)
            for p, (c0, c1) in enumerate(pan):
                t = R[c0:c1] - S[c0:c1, off:c0] @ R[off:c0]
                R[c0:c1] = Ys[p] @ t
                if R is W and off == 0 and p == 0:
                    if fault == "w_tile" and nb >= 32:
                        R[:min(16, c1), 16:32] = R[:min(16, c1), 0:16]
                    if fault == "swap" and nb >= 16 and c1 >= 16:
                        R[:16, :16] = R[:16, :16].T.copy()
        if end < m:
            L21T = S[off:end, end:]
            S[end:, end:] -= L21T.T @ L21T
            W[end:] -= L21T.T @ W[off:end]
    return S, W
