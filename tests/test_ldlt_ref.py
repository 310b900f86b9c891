"""The long-double restatement of the pivoted LDL^T update (tests/ldlt_ref.py) against independent routes: numpy.linalg in double,
residuals, the Cholesky solve on positive definite problems, and a hand-made pivot order.  No GPU."""
import numpy as np
import pytest

from tests import ldlt_ref as R

LD = np.longdouble
SIZES = [1, 2, 17, 64, 150, 330]


def _indefinite(m, seed):
    """random symmetric indefinite S with a spread of eigenvalue signs and a well separated diagonal"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(0, 1, (m, m)))
    lam = rng.uniform(0.5, 2.0, m) * np.where(rng.uniform(0, 1, m) < 0.4, -1.0, 1.0)
    S = (Q * lam) @ Q.T
    return (S + S.T) / 2


@pytest.mark.parametrize("m", SIZES)
def test_factor_reproduces_S_and_solve_has_a_small_residual(m):
    S = _indefinite(m, 100 + m)
    rng = np.random.default_rng(m)
    B = rng.normal(0, 1, (m, 5))
    L, D, perm, _ = R.ldlt_factor(S)
    assert np.array_equal(np.sort(perm), np.arange(m))
    assert np.array_equal(np.triu(L, 1), np.zeros((m, m))) and np.array_equal(np.diag(L), np.ones(m))
    # P_pi S P_pi^T = L D L^T: the backward error of a long-double factorisation, gamma_m in units of 2^-64, on |L||D||L^T|
    rec = (L * D[None, :]) @ L.T
    scale = (np.abs(L) * np.abs(D)[None, :]) @ np.abs(L).T
    u_ld = float(np.finfo(LD).eps) / 2
    assert (np.abs(rec - np.asarray(S, LD)[np.ix_(perm, perm)]) <= 2 * (m + 1) * u_ld * scale + 1e-300).all()
    X = R.ldlt_solve(L, D, perm, B)
    # S X = B: residual against the double-precision product, bounded by what forming S X in double costs + the solve's own error
    res = np.abs(S @ np.asarray(X, np.float64) - B)
    bound = 4 * R.gamma(m + 2) * (np.abs(S) @ np.abs(np.asarray(X, np.float64)) + np.abs(B))
    assert (res <= bound).all(), float((res / bound).max())
    # the independent route: LAPACK's LU in double, to its own forward error (cond * u)
    Xd = np.linalg.solve(S, B)
    cond = np.linalg.cond(S)
    assert np.abs(np.asarray(X, np.float64) - Xd).max() <= 8 * m * cond * R.U * np.abs(Xd).max()


def test_reads_the_lower_triangle_only():
    S = _indefinite(17, 5)
    junk = np.tril(S) + np.triu(np.full((17, 17), np.nan), 1)
    a, b = R.ldlt_factor(S), R.ldlt_factor(junk)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("m", SIZES)
def test_positive_definite_solve_equals_cholesky(m):
    rng = np.random.default_rng(7 * m)
    A = rng.normal(0, 1, (m, m + 3)); S = A @ A.T + 0.1 * np.eye(m)
    B = rng.normal(0, 1, (m, 4))
    L, D, perm, _ = R.ldlt_factor(S)
    assert (D > 0).all() and R.d_info(D) == (0, 0)
    X = np.asarray(R.ldlt_solve(L, D, perm, B), np.float64)
    C = np.linalg.cholesky(S)
    Xc = np.linalg.solve(C.T, np.linalg.solve(C, B))
    assert np.abs(X - Xc).max() <= 8 * m * np.linalg.cond(S) * R.U * np.abs(Xc).max()


def test_pivot_order_of_a_hand_made_example():
    """diag 1, -5, 3, 2 with one coupling: step 0 takes -5 (index 1); its elimination turns entry 3 (coupled to it by 4) from
    2 into 2 - 16 / (-5) = 5.2, the new largest (index 3), which is not coupled to the rest; then 3 (index 2), then 1 (index 0)."""
    S = np.diag([1.0, -5.0, 3.0, 2.0])
    S[3, 1] = S[1, 3] = 4.0
    L, D, perm, gaps = R.ldlt_factor(S)
    assert perm.tolist() == [1, 3, 2, 0]
    assert np.allclose(np.asarray(D, np.float64), [-5.0, 5.2, 3.0, 1.0], rtol=1e-15, atol=0)
    assert R.d_info(D) == (1, 0)
    assert float(L[1, 0]) == pytest.approx(-0.8, rel=1e-15)            # row 3 of S, now row 1: 4 / -5
    assert gaps[0] == pytest.approx(0.4) and gaps[1] == pytest.approx((5.2 - 3) / 5.2)


def test_tie_takes_the_first_and_zero_pivots_solve_to_zero():
    L, D, perm, gaps = R.ldlt_factor(np.diag([2.0, -2.0, 2.0]))
    assert perm.tolist() == [0, 1, 2] and gaps[0] == 0.0
    S = np.zeros((3, 3)); S[0, 0] = 4.0
    L, D, perm, _ = R.ldlt_factor(S)
    assert R.d_info(D) == (0, 2)
    X = R.ldlt_solve(L, D, perm, np.array([8.0, 1.0, 1.0]))
    assert np.asarray(X, np.float64).tolist() == [2.0, 0.0, 0.0]


@pytest.mark.parametrize("N,m,bad", [(120, 40, 7), (60, 17, 3)])
def test_full_update_against_double_precision_algebra(N, m, bad):
    """dx and the new P of an update from an indefinite covariance, against numpy.linalg.solve on the same S"""
    rng = np.random.default_rng(N + m)
    Bm = rng.normal(0, 1, (N, N)); P = Bm @ Bm.T * 1e-3 + np.diag(rng.uniform(1e-8, 1e-2, N))
    H = rng.normal(0, 1, (m, N)) * (rng.uniform(0, 1, (m, N)) < 0.2); H[:, :15] = 0
    r = rng.normal(0, 0.01, m)
    H[:, 30] = 0.0; H[bad, :] = 0.0; H[bad, 30] = 1.0
    P[30, :] = 0.0; P[:, 30] = 0.0; P[30, 30] = -1.0
    s2 = 0.008 ** 2
    ref = R.ekf_update_ldlt(P, H, r, s2)
    assert ref["info"] == (1, 0)
    assert float(ref["D"][list(ref["perm"]).index(bad)]) == pytest.approx(-1.0 + s2, rel=1e-12)     # row `bad` is decoupled: its pivot is S[bad, bad]
    S = H @ P @ H.T + s2 * np.eye(m)
    X = np.linalg.solve(S, H @ P)
    dx = X.T @ r; Pn = P - X.T @ (H @ P); Pn = (Pn + Pn.T) / 2
    tol = 8 * m * np.linalg.cond(S) * R.U
    assert np.abs(np.asarray(ref["dx"], np.float64) - dx).max() <= tol * np.abs(dx).max()
    assert np.abs(np.asarray(ref["P"], np.float64) - Pn).max() <= tol * np.abs(P).max()
    assert np.array_equal(ref["P"], ref["P"].T)
    bdx, bP = R.forward_bound(P, H, r, s2, ref)
    assert np.isfinite(np.asarray(bdx, np.float64)).all() and (bP >= 0).all()
