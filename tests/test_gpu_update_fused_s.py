"""The measurement update with S formed inside the H P launch (larvio_amd/csrc/be_linalg.hip: k_hp_splanes writes [HP | r] and S as ordered
partial planes, one per block of state columns; k_chol_fused's loader adds the planes and sigma^2 while it loads), through lvk_ekf_update
against a NumPy float64 restatement of the update.  The fused pair is selected by LVK_UPDATE_FUSED_S=1, read once per process (it is
built and kept, not the default: DESIGN.md 5.0c), so every case runs in two child processes - one with the switch on, one with it
off - that each write what they computed to a file (the worker at the bottom of this module); the tests compare both files with
the reference.  With the switch on m <= 160 takes the fused pair, taller updates the four-launch path; both are held
to the bounds tests/test_gpu_backend.py::test_ekf_update_matches_oracle applies to this entry point (DX_REL, P_REL below are its
constants).  Shapes sit on the edges of the new code: 16-row tiles, 32-row panels, the 160-row cap, a ragged last column block
(n = 215: blocks of 80, 80 and 55 columns; n = 23: one block of 23), a column block wider than one pass (n = 300), padded operands."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DX_REL, P_REL = 1e-9, 1e-10          # tests/test_gpu_backend.py::test_ekf_update_matches_oracle
SIGMA2 = 0.008 ** 2


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def problem(seed, n, m):
    """P random SPD, H random and sparse with whole column blocks zero (the filter's rows see a few clones each), r"""
    rng = np.random.default_rng(seed)
    Bm = rng.normal(0, 1, (n, n)); P = Bm @ Bm.T * 1e-3 + np.diag(rng.uniform(1e-8, 1e-2, n))
    H = rng.normal(0, 1, (m, n)) * (rng.uniform(0, 1, (m, n)) < 0.2)
    H[:, :min(15, n // 2)] = 0
    for lo in range(21, n - 6, 48):
        H[:, lo:lo + 6] = 0
    r = rng.normal(0, 0.01, m)
    return P, H, r


def update_ref(P, H, r, sigma2):
    """S = H P H^T + sigma^2 I = L L^T ; W = L^-1 H P ; dx = W^T L^-1 r ; P <- P - W^T W, symmetrised (float64 throughout)"""
    HP = H @ P
    S = HP @ H.T + sigma2 * np.eye(len(H))
    L = np.linalg.cholesky(0.5 * (S + S.T))
    W = np.linalg.solve(L, HP); w = np.linalg.solve(L, r)
    Pn = P - W.T @ W
    return W.T @ w, 0.5 * (Pn + Pn.T)


_REF = {}


def case(n, m):
    if (n, m) not in _REF:
        P, H, r = problem(1000 * n + m, n, m)
        _REF[(n, m)] = (P, H, r) + update_ref(P, H, r, SIGMA2)
    return _REF[(n, m)]


def check(tag, dx_g, P_g, dx_o, P_o):
    e_dx, e_P = _rel(dx_g, dx_o), _rel(P_g, P_o)
    print(f"{tag}: dx {e_dx:.3e} (bound {DX_REL:g})  P {e_P:.3e} (bound {P_REL:g})")
    assert e_dx < DX_REL and e_P < P_REL, (tag, e_dx, e_P)



# m <= 160: the fused pair (tile edges 15/16/17, panel edges 31/32/33, the cap 159/160); 161 and 200: the unfused path whatever the switch
GRID = [(n, m) for n in (23, 215) for m in (1, 15, 16, 17, 31, 32, 33, 127, 159, 160, 161, 200)]
# n = 300: 19 column tiles in blocks of 7, 7 and 5 - wider than one pass of five tiles, the last block and its last tile ragged;
# 241: the first width of two passes; 16: a single full tile, one plane; 48: three planes of one tile each
EDGES = [(300, 40), (241, 33), (16, 5), (48, 160)]
PADDED = [(215, 127, 226), (215, 160, 233), (23, 17, 29), (215, 161, 226)]       # ldp = ldh = ld > n, rows not 32-byte aligned
REPEAT = [(215, 127), (215, 160), (23, 33)]
SINGULAR = [(23, 20), (215, 100)]
NEIGHBOUR = (215, 127)


def singular_problem(n, m):
    """sigma^2 = 0 and two equal rows of H: S is singular.  Every number is a small integer (P = 4 I, the rows of H distinct unit
    vectors but for rows 0 and 1), so every sum is exact in any order, the first pivot's inverse root is exactly 1/2 and the second
    pivot exactly 0"""
    assert m <= n
    P = 4.0 * np.eye(n); H = np.zeros((m, n))
    H[np.arange(m), np.arange(m)] = 1.0
    H[1] = H[0]
    return P, H, np.ones(m)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """what a process with LVK_UPDATE_FUSED_S=1 ("on") and one with LVK_UPDATE_FUSED_S=0 ("off") computed for every case"""
    d = tmp_path_factory.mktemp("fused_s")
    got = {}
    for name, val in (("on", "1"), ("off", "0")):
        env = dict(os.environ, LVK_UPDATE_FUSED_S=val)
        path = str(d / (name + ".npz"))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
        got[name] = np.load(path)
    return got


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("n,m", GRID + EDGES)
def test_update_matches_numpy(runs, switch, n, m):
    _, _, _, dx_o, P_o = case(n, m)
    dx_g, P_g = runs[switch][f"dx_{n}_{m}"], runs[switch][f"P_{n}_{m}"]
    check(f"{switch} n {n} m {m}", dx_g, P_g, dx_o, P_o)
    assert np.array_equal(P_g, P_g.T)


@pytest.mark.parametrize("n,m", GRID + EDGES)
def test_switch_on_against_off(runs, n, m):
    """the two routes on the same inputs: their mutual difference is printed (another summation order of S, nothing bit-pinned) and
    held to no more than the bound allows - each lies within it around the reference, so within twice the bound of the other"""
    d_dx = _rel(runs["on"][f"dx_{n}_{m}"], runs["off"][f"dx_{n}_{m}"]); d_P = _rel(runs["on"][f"P_{n}_{m}"], runs["off"][f"P_{n}_{m}"])
    print(f"LVK_UPDATE_FUSED_S=1 against 0, n {n} m {m}: dx {d_dx:.3e}  P {d_P:.3e}")
    assert d_dx < 2 * DX_REL and d_P < 2 * P_REL
    if m > 160:                                     # taller than the fused launch of the Cholesky: the switch changes nothing
        assert d_dx == 0 and d_P == 0


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("n,m,ld", PADDED)
def test_update_padded_operands(runs, switch, n, m, ld):
    """NaN in the padding: inside the bound, the same bits as the packed call, padding neither read (NaN would spread) nor written"""
    R = runs[switch]
    _, _, _, dx_o, P_o = case(n, m)
    dx_s, buf = R[f"pdx_{n}_{m}_{ld}"], R[f"pP_{n}_{m}_{ld}"]
    check(f"{switch} n {n} m {m} ld {ld}", dx_s, buf[:, :n], dx_o, P_o)
    assert dx_s.tobytes() == R[f"dx_{n}_{m}"].tobytes() and buf[:, :n].tobytes() == R[f"P_{n}_{m}"].tobytes()
    assert np.isnan(buf[:, n:]).all()


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("n,m", REPEAT)
def test_update_is_reproducible_bit_for_bit(runs, switch, n, m):
    """one update twice on one context: which column block lands in which plane, and the order the planes are added in, depend on
    indices alone"""
    R = runs[switch]
    assert R[f"dx_{n}_{m}"].tobytes() == R[f"dx2_{n}_{m}"].tobytes() and R[f"P_{n}_{m}"].tobytes() == R[f"P2_{n}_{m}"].tobytes()


@pytest.mark.parametrize("switch", ["on", "off"])
@pytest.mark.parametrize("n,m", SINGULAR)
def test_singular_innovation_is_reported_and_leaves_P_alone(runs, switch, n, m):
    """singular_problem: the factor workgroup reports row 1 in its report words, the call returns LVK_ERR_NUMERIC (5, include/lvk_c.h)
    with that pivot in its message, the gated last launch writes nothing, and the context goes on working"""
    R = runs[switch]
    st, pivot_named, unchanged = R[f"sing_{n}_{m}"]
    assert st == 5 and pivot_named == 1 and unchanged == 1, (st, pivot_named, unchanged, str(R[f"singmsg_{n}_{m}"]))
    _, _, _, dx_o, P_o = case(n, 17)
    check(f"{switch} after the report, n {n}", R[f"singdx_{n}_{m}"], R[f"singP_{n}_{m}"], dx_o, P_o)


@pytest.mark.parametrize("switch", ["on", "off"])
def test_lds_optin_neighbours_in_the_new_order(runs, switch):
    """tests/test_gpu_lds_optin.py's neighbour case with the fused pair, the first thing the worker does on its fresh context: an
    update (k_hp_splanes' static LDS, k_chol_fused's ~144 KB opt-in), then a register QR node of 200 x 40 (its own ~70 KB opt-in, held
    to that file's bounds inside the worker), then the update again"""
    R = runs[switch]
    _, _, _, dx_o, P_o = case(*NEIGHBOUR)
    assert int(R["nb_qr_ok"]) == 1, str(R["nb_qr_msg"])
    for k in (1, 2):
        check(f"{switch} update {k} of 2", R[f"nb{k}_dx"], R[f"nb{k}_P"], dx_o, P_o)


def _worker(path):
    """every case of this module on one fresh context, under whatever LVK_UPDATE_FUSED_S this process was started with"""
    import larvio_amd
    from larvio_amd import larvio as lv
    from larvio_amd._lib import lib
    from tests.test_gpu_lds_optin import _compress
    ctx = larvio_amd.Context()
    out = {}
    P, H, r, _, _ = case(*NEIGHBOUR)
    out["nb1_dx"], out["nb1_P"] = lv.ekf_update(ctx, P, H, r, SIGMA2)
    try:
        _compress(ctx, 40, 200)
        out["nb_qr_ok"], out["nb_qr_msg"] = 1, ""
    except AssertionError as e:
        out["nb_qr_ok"], out["nb_qr_msg"] = 0, repr(e)
    out["nb2_dx"], out["nb2_P"] = lv.ekf_update(ctx, P, H, r, SIGMA2)
    for n, m in GRID + EDGES:
        P, H, r, _, _ = case(n, m)
        out[f"dx_{n}_{m}"], out[f"P_{n}_{m}"] = lv.ekf_update(ctx, P, H, r, SIGMA2)
        if (n, m) in REPEAT:
            out[f"dx2_{n}_{m}"], out[f"P2_{n}_{m}"] = lv.ekf_update(ctx, P, H, r, SIGMA2)
    for n, m, ld in PADDED:
        P, H, r, _, _ = case(n, m)
        out[f"pdx_{n}_{m}_{ld}"], out[f"pP_{n}_{m}_{ld}"] = lv.ekf_update(ctx, P, H, r, SIGMA2, ld=ld)
    for n, m in SINGULAR:
        P, H, r = singular_problem(n, m)
        dP, dH, dr, ddx = ctx.to_device(P), ctx.to_device(H), ctx.to_device(r), ctx.alloc(8 * n)
        st = lib().lvk_ekf_update(ctx.h, lv._p(dP), n, n, lv._p(dH), n, m, lv._p(dr), 0.0, lv._p(ddx))
        msg = lib().lvk_last_error(ctx.h).decode()
        out[f"sing_{n}_{m}"] = np.array([st, int("not positive definite (pivot 1)" in msg), int(ctx.to_host(dP, np.float64, P.shape).tobytes() == P.tobytes())])
        out[f"singmsg_{n}_{m}"] = msg
        P, H, r, _, _ = case(n, 17)
        out[f"singdx_{n}_{m}"], out[f"singP_{n}_{m}"] = lv.ekf_update(ctx, P, H, r, SIGMA2)
    ctx.close()
    np.savez(path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from tests import test_gpu_update_fused_s as me          # one copy of the problem cache, whoever imports it
    me._worker(sys.argv[1])
