"""The measurement update through an LDL^T factorisation with diagonal pivoting, restated in numpy.longdouble: what
lvk_ekf_update_ldlt (larvio_amd/csrc/be_ldlt.hip) computes in FP64 and what the reference runs as S.ldlt().solve(H P)
(larvio.cpp:1456-1460, 1578-1594).  The algorithm is LDLTx of oracle/ref_shim2/lvref_eigen2.hpp:

    P_pi S P_pi^T = L D L^T; at step k the remaining diagonal entry of largest magnitude becomes the pivot - the FIRST one on an exact
    tie (the tie rule of this file and of the kernel) - and rows/columns k and p are swapped symmetrically; only the lower triangle
    of S is read.  A zero pivot leaves a zero column of L.
    X = P_pi^T L^-T D^-1 L^-1 P_pi B, where a D entry of magnitude <= DBL_MIN gives a zero component instead of a division.
    K = X[:, :n]^T for B = [H P | r];  dx = K r;  P <- (I - K H) P;  P <- (P + P^T) / 2.

Everything here is long double (x87 extended, u = 2^-64, on the machines the suite runs on), so that against FP64 results it stands for
the exact answer.  The error bound of the FP64 computation lives here too (forward_bound): it is derived, not measured."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                           # FP64 unit roundoff
TINY = np.finfo(np.float64).tiny         # DBL_MIN: the solve's zero rule


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a length-k sum or dot product in FP64, whatever its order"""
    return k * U / (1.0 - k * U)


def ldlt_factor(S):
    """-> L (unit lower, m x m), D (m), perm (row i of the factor is row perm[i] of S), gaps (per step: (best - runner-up) / best of the
    remaining |diagonal|; inf for the last step or a zero block).  Reads the lower triangle of S only."""
    S = np.asarray(S, LD)
    m = S.shape[0]
    A = np.tril(S) + np.tril(S, -1).T                      # the symmetric matrix the lower triangle stands for
    perm = np.arange(m)
    D = np.zeros(m, LD)
    gaps = np.full(m, np.inf)
    for k in range(m):
        dg = np.abs(np.diag(A)[k:])
        p = k + int(np.argmax(dg))                         # numpy's argmax returns the first maximum
        if m - k > 1:
            rest = np.delete(dg, p - k)
            if dg[p - k] > 0:
                gaps[k] = float((dg[p - k] - rest.max()) / dg[p - k])
        if p != k:
            A[[k, p], :] = A[[p, k], :]
            A[:, [k, p]] = A[:, [p, k]]
            perm[[k, p]] = perm[[p, k]]
        d = A[k, k]
        D[k] = d
        if d == 0:
            A[k + 1:, k] = 0
            continue
        l = A[k + 1:, k] / d
        A[k + 1:, k + 1:] -= np.outer(l, l * d)
        A[k + 1:, k] = l
    L = np.tril(A, -1) + np.eye(m, dtype=LD)
    return L, D, perm, gaps


def ldlt_solve(L, D, perm, B):
    """X with S X = B, through P_pi^T L^-T D^-1 L^-1 P_pi; zero component where |D| <= DBL_MIN"""
    B = np.asarray(B, LD)
    m = L.shape[0]
    y = B[perm].copy() if B.ndim == 2 else B[perm].copy()
    for i in range(1, m):
        y[i] -= L[i, :i] @ y[:i]
    ok = np.abs(D) > TINY
    scale = np.where(ok, 1 / np.where(ok, D, 1), 0)
    y = y * (scale[:, None] if y.ndim == 2 else scale)
    for i in range(m - 2, -1, -1):
        y[i] -= L[i + 1:, i] @ y[i + 1:]
    X = np.empty_like(y)
    X[perm] = y
    return X


def d_info(D):
    """(negative, zero) D entries, as lvk_ekf_update_ldlt reports them"""
    Dd = np.asarray(D, np.float64)
    return int((Dd < -TINY).sum()), int((np.abs(Dd) <= TINY).sum())


def ekf_update_ldlt(P, H, r, sigma2):
    """-> dict(dx, P, info, perm, gaps, and the intermediates HP, S, L, D, X the bound needs), all long double"""
    P = np.asarray(P, LD); H = np.asarray(H, LD); r = np.asarray(r, LD)
    m, n = H.shape
    HP = H @ P
    S = HP @ H.T + LD(sigma2) * np.eye(m, dtype=LD)
    L, D, perm, gaps = ldlt_factor(S)
    X = ldlt_solve(L, D, perm, np.concatenate([HP, r[:, None]], axis=1))[:, :n]
    dx = X.T @ r
    Pn = P - X.T @ HP
    Pn = (Pn + Pn.T) / 2
    return dict(dx=dx, P=Pn, info=d_info(D), perm=perm, gaps=gaps, HP=HP, S=S, L=L, D=D, X=X)


def forward_bound(P, H, r, sigma2, ref):
    """Componentwise bounds (bdx, bP) on |computed - exact| for the FP64 computation of ekf_update_ldlt in ANY summation order, from
    the standard rounding-error analysis (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.: (3.5) for dot products,
    Theorems 8.5 and 10.4 / section 11.1 for substitution and the LDL^T solve), first order in u with the quantities of the
    long-double restatement `ref`:
      HP^ = H P + E1,                 |E1| <= gamma_n |H||P|
      S^  = S + E2,                   |E2| <= gamma_n |H||P||H^T| + gamma_{n+1} (|HP||H^T| + sigma2 I)
      (S^ + E3) X^ = HP^ (per column) |E3| <= gamma_{3m+1} Pi^T |L||D||L^T| Pi      (factorisation + two substitutions + the D scaling)
      =>  |X^ - X| <= |S^-1| ((|E2| + |E3|) |X| + |E1|)  =: EX
      dx^ = X^T r:                    |ddx| <= EX^T |r| + gamma_m |X|^T |r|
      Pn^ = P - X^T HP:               |dPn| <= EX^T |HP| + |X|^T |E1| + gamma_{m+1} (|X|^T |HP| + |P|)
      (Pn^ + Pn^T) / 2:               the mean of the bound and its transpose, + u |Pn|
    The terms of second order in u are bounded by doubling the result (they are smaller than the first-order ones as long as the
    bound itself is small against the solution, which test code asserts where it uses this).  |S^-1| comes from the restatement's
    own factors (solve of the identity)."""
    aP = np.abs(np.asarray(P, LD)); aH = np.abs(np.asarray(H, LD)); ar = np.abs(np.asarray(r, LD))
    m, n = aH.shape
    L, D, perm, X, HP = ref["L"], ref["D"], ref["perm"], ref["X"], ref["HP"]
    aX, aHP = np.abs(X), np.abs(HP)
    HaP = aH @ aP
    E1 = gamma(n) * HaP
    E2 = gamma(n) * (HaP @ aH.T) + gamma(n + 1) * (aHP @ aH.T + sigma2 * np.eye(m, dtype=LD))
    LDL = (np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T
    E3 = np.empty_like(LDL); E3[np.ix_(perm, perm)] = gamma(3 * m + 1) * LDL
    Sinv = np.abs(ldlt_solve(L, D, perm, np.eye(m, dtype=LD)))
    EX = Sinv @ ((E2 + E3) @ aX + E1)
    bdx = EX.T @ ar + gamma(m) * (aX.T @ ar)
    bP = EX.T @ aHP + aX.T @ E1 + gamma(m + 1) * (aX.T @ aHP + aP)
    bP = (bP + bP.T) / 2 + U * np.abs(ref["P"])
    return 2 * bdx, 2 * bP
