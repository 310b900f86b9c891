"""Helpers of the sequence comparators (tests/test_gpu_backend.py, tests/test_gpu_vio_driver.py): names of the state blocks and the
covariance error in correlation units."""
import numpy as np

CORR = 1e-5          # max |Pg - Po|_ij / sqrt(Po_ii Po_jj), the north_star's 1e-5 in correlation units


def block_name(x, leg, n_clones):
    """the state block of covariance row x: IMU part (leg = 22, or 46 with IMU intrinsics), clone, in-state feature"""
    if x < leg: return ("th", "v", "p", "bg", "ba", "th_ext", "t_ext", "td/imx")[min(x // 3, 7)]
    return f"clone{(x - leg) // 6}.{'th' if (x - leg) % 6 < 3 else 'p'}" if x < leg + 6 * n_clones else f"feat{x - leg - 6 * n_clones}"


def corr_error(Pg, Po, leg, n_clones):
    """max |Pg - Po|_ij / sqrt(Po_ii Po_jj): the covariance error in correlation units, which a small block (td, the extrinsics, an
    inverse depth) cannot hide behind the largest entry of P.  Rows whose variance is zero in Po (states the filter does not estimate,
    e.g. extrinsics and td with estimate_extrin / estimate_td off) have no scale: there Pg must equal Po exactly, and any difference -
    like a NaN anywhere - counts as an infinite error.  Returns (value, description of the worst entry)."""
    Pg = np.asarray(Pg, np.float64); Po = np.asarray(Po, np.float64)
    var = np.diag(Po)
    prod = np.outer(var, var)
    diff = np.abs(Pg - Po)
    scaled = prod > 0
    e = np.zeros_like(diff)
    e[scaled] = diff[scaled] / np.sqrt(prod[scaled])
    e[~scaled & (diff != 0)] = np.inf
    e[np.isnan(diff)] = np.inf
    ij = np.unravel_index(np.argmax(e), e.shape)
    n_zero = int((var <= 0).sum())
    at = (f"entry ({block_name(ij[0], leg, n_clones)},{block_name(ij[1], leg, n_clones)}) = {Po[ij]:.3e} differs by {diff[ij]:.3e}; "
          f"variances {var[ij[0]]:.3e}, {var[ij[1]]:.3e}")
    if n_zero:
        at += f"; {n_zero} rows of zero variance, compared exactly"
    return float(e[ij]), at
