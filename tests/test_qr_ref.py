"""The CPU conditions of the QR stage tests (tests/test_gpu_qr_stages.py, restatement in tests/qr_ref.py): every case lands on the
kernel and specialisation it names, the reference itself is accurate on every case (tau_ref <= 1e-12, so the bound is never
vacuous), and the reference meets the structural claims the GPU tests make of the kernels.  No GPU."""
import numpy as np
import pytest

from tests import qr_ref as Q

TAU_MAX = 1e-12


def _plan(c):
    from larvio_amd import larvio as lv
    return lv.qr_plan(c["N"], c["groups"])


def _tau(H, r, Href, rref):
    return Q.pair_errors(Q.gram(Href, rref), Q.gram(H, r), Q.col_norms(H, r)).max()


@pytest.mark.parametrize("name", Q.GROUP_CASES)
def test_group_case_lands_on_its_kernel(name):
    c = Q.group_case(name)
    levels, final_rows = _plan(c)
    ks = Q.level_kernels(levels, c["N"])
    assert [k["kernel"] for k in ks] == c["kernels"], ks
    if "optin" in c:
        assert [k["optin"] for k in ks] == c["optin"], ks
    if "nodes" in c:
        assert [k["nodes"] for k in ks] == c["nodes"] and [k["copies"] for k in ks] == c["copies"], ks
    if name.startswith(("reg_", "lds_", "gate_")):                  # one group, one node of exactly that shape
        (R, cols), = c["groups"]
        (b,), = [L["blocks"] for L in levels]
        assert not b["copy"] and b["in_rows"] == R and b["ncols"] == len(cols)
    if name.startswith("mixed_"):                                   # RPL set by one node, the widest union by another, copies of 2 rows
        nodes = [b for b in levels[0]["blocks"] if not b["copy"]]
        tallest, widest = max(nodes, key=lambda b: b["in_rows"]), max(nodes, key=lambda b: b["ncols"])
        assert tallest is not widest and tallest["in_rows"] > widest["in_rows"] and widest["ncols"] > tallest["ncols"]
        small = min(nodes, key=lambda b: b["in_rows"])
        assert small["in_rows"] <= 32 and small["ncols"] < ks[0]["max_cols"]
        assert [b["in_rows"] for b in levels[0]["blocks"] if b["copy"]] == [2] * c["copies"][0]
    assert final_rows < len(c["H"])


def test_register_cases_cover_the_kernel_edges():
    """k_qr_sparse_reg: both RPL specialisations, every chunk handover (steps 15 / 31 / 47) in each, the column counts and row counts
    the issue of these tests names"""
    ncs = {nc for nc, _ in Q.REG_NODES}
    assert {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63} <= ncs
    Rs = {R for _, R in Q.REG_NODES}
    assert {16, 17, 64, 65, 127, 128, 129, 255, 256} <= Rs and any(R == nc + 1 for nc, R in Q.REG_NODES)
    for small in (True, False):
        cases = [(nc, R) for nc, R in Q.REG_NODES if (R <= 128) == small]
        for h in (15, 31, 47):                                       # a handover followed by a further step, and one that ends the node
            assert any(nc > h + 1 for nc, _ in cases) and any(nc == h + 1 for nc, _ in cases)


def test_dense_cases_hit_the_chunk_and_panel_edges():
    geo = {rc: Q.dense_geometry(*rc) for rc in Q.DENSE}
    # CH = 512 (NB = 32): one full chunk, one row over, two chunks and a row, a last chunk with fewer rows than NB
    assert geo[(512, 40)][:2] == (32, 512) and geo[(512, 40)][2][0]["nch"] == 1 and geo[(512, 40)][2][0]["last"] == 512
    assert geo[(513, 40)][2][0]["nch"] == 2 and geo[(513, 40)][2][0]["last"] == 1
    assert geo[(1025, 64)][2][0]["nch"] == 3 and geo[(1025, 64)][2][0]["last"] == 1
    assert geo[(543, 33)][2][0]["nch"] == 2 and geo[(543, 33)][2][0]["last"] == 31 < 32
    # CH = 1024 (NB = 16)
    assert geo[(8193, 33)][:2] == (16, 1024) and geo[(8193, 33)][2][0]["last"] == 1
    assert geo[(9216, 17)][:2] == (16, 1024) and [p["last"] for p in geo[(9216, 17)][2]] == [1024, 1008]
    assert geo[(9217, 48)][2][0]["nch"] == 10 and geo[(9217, 48)][2][0]["last"] == 1
    # the chunk count drops from three to two between panels 0 and 1
    assert [p["nch"] for p in geo[(1044, 64)][2]] == [3, 2]
    # the 65,536-row capacity: NB = 16, 64 chunks
    assert geo[(65536, 17)][:2] == (16, 1024) and geo[(65536, 17)][2][0]["nch"] == 64
    # panel edges: a last panel narrower than NB, a last panel exactly NB wide with only the residual right of it
    last = [geo[(700, c)][2][-1] for c in Q.DENSE_PANEL_COLS]
    assert any(p["nb"] < 32 for p in last) and any(p["nb"] == 32 and p["trailing"] == 0 for p in last)
    # few rows left in the last panel: rows = cols + 1, cols + 2
    for c in Q.DENSE_PANEL_COLS:
        for rows in (c + 1, c + 2):
            p = geo[(rows, c)][2][-1]
            assert rows - p["j0"] <= p["nb"] + 2 and p["nch"] == 1


@pytest.mark.parametrize("name", Q.GROUP_CASES)
def test_group_reference_is_accurate_and_structured(name):
    c = Q.group_case(name)
    levels, final_rows = _plan(c)
    Href, rref = Q.emulate(levels, c["H"], c["r"])
    assert len(Href) == final_rows
    assert Q.structural_violations(levels, c["H"], c["r"], Href, rref) == []
    tau = _tau(c["H"], c["r"], Href, rref)
    assert tau <= TAU_MAX, tau


@pytest.mark.parametrize("rows,cols", Q.DENSE)
def test_dense_reference_is_accurate(rows, cols):
    H, r = Q.dense_case(rows, cols)
    Href, rref = Q.reference_dense(H, r)
    assert Href.shape == (cols, cols) and np.all(Href[np.tril_indices(cols, -1)] == 0)
    tau = _tau(H, r, Href, rref)
    assert tau <= TAU_MAX, tau


@pytest.mark.parametrize("kernel", Q.NEGLIGIBLE_KERNELS)
@pytest.mark.parametrize("side", ["below", "above"])
def test_negligible_cases(kernel, side):
    """the tiny column is below QR_NEGLIGIBLE at every step (its whole sum of squares is) or far above it at its own step (R_kk^2 of the
    reference); the case runs in the kernel it names; the reference is accurate on it"""
    H, r, k, groups, N = Q.negligible_case(kernel, side)
    ss = float((H[:, k].astype(Q.LD) ** 2).sum())
    if groups is None:
        Href, rref = Q.reference_dense(H, r)
        rkk = Href[k, k]
    else:
        from larvio_amd import larvio as lv
        levels, _ = lv.qr_plan(N, groups)
        assert [x["kernel"] for x in Q.level_kernels(levels, N)] == [{"reg": "reg8", "lds": "lds"}[kernel]]
        Href, rref = Q.emulate(levels, H, r)
        rkk = Href[groups[0][1].index(k), k]
    if side == "below":
        assert ss <= Q.QR_NEGLIGIBLE
    else:
        assert rkk ** 2 > 1e10 * Q.QR_NEGLIGIBLE
    tau = _tau(H, r, Href, rref)
    assert tau <= TAU_MAX, tau
