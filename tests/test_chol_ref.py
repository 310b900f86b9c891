"""CPU self-test of tests/chol_ref.py: the restatement is what it says, the derived bound holds for a plain FP64 emulation of the blocked
algorithm on every problem of the GPU stage tests (not too tight), planted faults exceed it (not too loose), and every problem meets
the side condition under which the first-order analysis stands - all before anything runs on a GPU."""
import numpy as np
import pytest

from tests import chol_ref as R


def test_restatement_reproduces_its_inputs():
    S, B, ref, _ = R.find_problem(97, 33)
    L, W, X = ref["L"], ref["W"], ref["X"]
    Sl = np.asarray(S, R.LD)
    scale = float(np.abs(Sl).max())
    assert float(np.abs(L @ L.T - Sl).max()) < 1e-17 * scale * 97
    assert float(np.abs(L @ W - np.asarray(B, R.LD)).max()) < 1e-17 * float(np.abs(B).max()) * 97
    assert float(np.abs(Sl @ X - np.asarray(B, R.LD)).max()) < 1e-15 * float(np.abs(B).max()) * 97
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    assert float(np.abs(ref["G"] - ref["G"].T).max()) == 0.0


def test_problems_are_filter_like():
    S, B = R.problem(129, 33, 5)
    assert np.array_equal(S, S.T) and B.shape == (129, 33)
    assert np.linalg.eigvalsh(S).min() > 0.5 * R.SIGMA ** 2
    col = np.abs(B[:, :32]).max(axis=0)
    assert col.max() / col.min() > 1e3                      # columns of H P carry the spread of the variances


def test_stored_mask_and_extract_L():
    m = 200
    M = R.stored_mask(m)
    assert not M[31, 0] and M[32, 0] and M[32, 31] and not M[63, 32] and M[160, 159] and M[199, 0] and not M[191, 160] and not M[0, 32]
    S = np.arange(m * m, dtype=np.float64).reshape(m, m)
    Lx = R.extract_L(S, m)
    assert Lx[40, 3] == S[40, 3] and Lx[170, 3] == S[3, 170] and Lx[190, 161] == 0 and Lx[192, 161] == S[192, 161] and Lx[3, 40] == 0


@pytest.mark.parametrize("m,nbcols", R.ALL_CASES)
def test_fp64_emulation_stays_within_the_bound(m, nbcols):
    S, B, ref, bnd = R.find_problem(m, nbcols)              # find_problem asserts the side condition (no case is left out)
    assert R.side_condition(ref, bnd)
    Se, We = R.emulate(S, B)
    rW, rG, rL = R.ratios(We, R.extract_L(Se, m), ref, bnd)
    print(f"m {m} nbcols {nbcols}: emulation |error| / bound: W {rW:.3e} G {rG:.3e} L {rL:.3e}   eps {bnd['eps']:.2e}  "
          f"bound / max: W {bnd['W'].max() / float(np.abs(ref['W']).max()):.2e} G {bnd['G'].max() / float(np.abs(ref['G']).max()):.2e}")
    assert rW <= 1.0 and rG <= 1.0 and rL <= 1.0, (rW, rG, rL)


@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("m,nbcols", [(97, 33), (160, 33), (65, 129), (225, 33)])
def test_planted_faults_exceed_the_bound(m, nbcols, fault):
    S, B, ref, bnd = R.find_problem(m, nbcols)
    Se, We = R.emulate(S, B, fault=fault)
    rW, rG, rL = R.ratios(We, R.extract_L(Se, m), ref, bnd)
    print(f"m {m} nbcols {nbcols} {fault}: |error| / bound: W {rW:.3e} G {rG:.3e} L {rL:.3e}")
    assert rW > 1.0 and rG > 1.0, (rW, rG)
    if fault in ("drop_chunk", "y_f32"):                    # faults of the factorisation also show in the stored blocks of L
        assert rL > 1.0, rL


def test_indefinite_problem_has_its_first_bad_pivot_where_asked():
    for bad in R.REPORT_BAD:
        S, _ = R.indefinite_problem(bad)
        with pytest.raises(ValueError, match=f"pivot {bad} "):
            R.cholesky(S)
