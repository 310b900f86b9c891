"""The dynamic-LDS opt-in cache of a context (LVK_LDS_OPTIN, larvio_amd/csrc/lvk_internal.h) is keyed on the kernel: what one kernel has
asked for never stands in for another's request.  k_chol_fused asks for a fixed ~144 KB; the register QR kernel k_qr_sparse_reg<16, 1>
asks for what its largest node needs, ~70 KB for 200 rows x 40 columns (the smallest such node above the 64 KB every kernel may use)
and ~136 KB for 256 x 63.  On a context of its own - the shared one has already seen other launches - a compression, an update and a
larger compression run in both orders; the compressions are held to the bounds of tests/qr_ref.py as in test_gpu_qr_stages.py, the
update to the oracle as in test_gpu_backend.py::test_ekf_update_matches_oracle."""
import numpy as np
import pytest

from tests import qr_ref as Q
from tests.test_gpu_backend import _rel, _update_problem
from tests.test_gpu_qr_stages import _errors

pytestmark = pytest.mark.gpu


def _compress(ctx, nc, R):
    from larvio_amd import larvio as lv
    c = Q.reg_node_case(nc, R)
    H, r = c["H"], c["r"]
    levels, final_rows = lv.qr_plan(c["N"], c["groups"])
    k = Q.level_kernels(levels, c["N"])
    assert [x["kernel"] for x in k] == ["reg16"] and k[0]["optin"], k          # one register node that needs the opt-in
    Hc, rc = lv.compress_qr_groups(ctx, H, r, c["groups"])
    assert len(Hc) == final_rows < len(H)
    assert np.isfinite(Hc).all() and np.isfinite(rc).all()
    bad = Q.structural_violations(levels, H, r, Hc, rc)
    assert not bad, bad[:8]
    Href, rref = Q.emulate(levels, H, r)
    e, b = _errors(f"optin reg_{nc}x{R} ({k[0]['lds']} bytes of LDS)", H, r, Hc, rc, Href, rref)
    assert e.max() <= b, np.unravel_index(np.argmax(e), e.shape)


def _update(ctx):
    from oracle import lvo_be
    from larvio_amd import larvio as lv
    N, m = 46, 9
    P, H, r = _update_problem(N + m, N, m)
    dx_o, P_o = lvo_be.ekf_update(P, H, r, 0.008 ** 2)
    dx_g, P_g = lv.ekf_update(ctx, P, H, r, 0.008 ** 2)
    assert _rel(dx_g, dx_o) < 1e-9
    assert _rel(P_g, P_o) < 1e-10
    assert np.array_equal(P_g, P_g.T)
    assert np.linalg.eigvalsh(P_g).min() > -1e-12


@pytest.mark.parametrize("order", ["small_chol_large", "large_chol_small"])
def test_one_kernels_opt_in_does_not_stand_in_for_anothers(order):
    import larvio_amd
    steps = [lambda c: _compress(c, 40, 200), _update, lambda c: _compress(c, 63, 256)]
    ctx = larvio_amd.Context()
    try:
        for step in (steps if order == "small_chol_large" else steps[::-1]):
            step(ctx)
    finally:
        ctx.close()
