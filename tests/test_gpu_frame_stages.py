"""The kernels a running front-end launches - k_fe_lk_both / k_fe_lk_pipe, k_fe_ransac_commit, k_fe_msg - one launch at a time through
their stage entries (lvk_fe_track_stage, lvk_fe_commit_stage, lvk_fe_msg_stage: the frame path's own launch code on host arrays) against
tests/fe_frame_ref.py, at the edges a sequence of natural frames reaches only by accident.  The cases are the tables of
tests/fe_frame_cases.py; tests/test_fe_frame_ref.py holds their reference half to the branch each was built for, without a GPU.
Everything is compared bit for bit (floats as their words), except the undistorted points of the fisheye camera, which go through tan():
rtol 2e-7, as test_undistort."""
import numpy as np
import pytest
from tests import fe_frame_ref as R
from tests import fe_frame_cases as K

pytestmark = pytest.mark.gpu
FILL = K.FILL


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.names is None else a.view(np.uint8)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


# =========================================================================== track stage
_PYR = {}


@pytest.fixture(scope="module", autouse=True)
def _release_pyramids():
    yield
    while _PYR:
        _PYR.popitem()[1].close()


def _gpu_pyramid(ctx, w, h, pair, which, win, levels):
    from larvio_amd import ops
    key = (w, h, pair, which, win, levels)
    if key not in _PYR:
        if len(_PYR) >= 8:
            _PYR.pop(next(iter(_PYR))).close()
        p = ops.Pyramid(ctx, w, h, win, levels - 1).build(K.frame_pair(w, h, pair)[which])
        p.orb_prepare()
        _PYR[key] = p
    return _PYR[key]


def _run_track(ctx, sc, sets, counters=(0, 0), variant=None, **kw):
    from larvio_amd import ops
    g0 = _gpu_pyramid(ctx, sc["w"], sc["h"], sc["pair"], 0, sc["win"], sc["levels"])
    g1 = _gpu_pyramid(ctx, sc["w"], sc["h"], sc["pair"], 1, sc["win"], sc["levels"])
    assert g0.n_levels == g1.n_levels == sc["levels"]
    model, intr, dist = sc["cam"]
    return ops.fe_track_stage(ctx, g0, g1, sets, sc["win"], sc["variant"] if variant is None else variant, sc["H"], model, intr, dist, fill=FILL, counters=counters, **kw)


def _check_track(got, ref, model, what):
    _same(got["status"], ref["status"], f"{what}: status")
    _same(got["curr"], ref["curr"], f"{what}: curr")
    if ref["desc"] is not None:
        _same(got["desc"], ref["desc"], f"{what}: desc")
    if model == 0:
        _same(got["und"], ref["und"], f"{what}: und")
    else:                                                     # slots nothing wrote hold the fill on both sides, bit for bit; the rest within test_undistort's tolerance
        unwritten = _bits(ref["und"]) == np.uint32(FILL * 0x01010101)
        assert np.array_equal(_bits(got["und"]) == np.uint32(FILL * 0x01010101), unwritten), f"{what}: which und slots were written"
        assert np.allclose(got["und"][~unwritten], ref["und"][~unwritten], rtol=2e-7, atol=0), f"{what}: und"


@pytest.mark.parametrize("name", list(K.TRACK_CASES))
def test_track_stage(gpu_ctx, name):
    sc = K.track_case(name)
    K.check_track_case(sc)
    ref = sc["ref"]
    _, outs, cnt = _run_track(gpu_ctx, sc, [dict(pts=sc["pts"], is_new=sc["is_new"], stored_desc=sc["stored"])], counters=(1000, 7))
    _check_track(outs[0], ref, sc["cam"][0], name)
    assert cnt == (1000 + ref["point_levels"], 7 + ref["iterations"])


@pytest.mark.parametrize("name,n,grid", [("pipe_L3_old_rot_shift", 37, 64), ("pipe_L3_old_rot_shift", 0, 8), ("both21_L2_new_I_half", 37, 64),
                                         ("both21_L2_new_I_half", 0, 8), ("both15_L4_old_I_half", 1, 2)])
def test_track_stage_blocks_beyond_n_write_nothing(gpu_ctx, name, n, grid):
    sc = K.track_case(name)
    pts = sc["pts"][:n]; stored = None if sc["is_new"] else sc["stored"][:n]
    ref = K.track_reference(sc, pts, sc["is_new"], stored, grid=grid)
    assert all((_bits(ref[k][n:]) == _bits(R.filled(1, ref[k].dtype, FILL))[0]).all() for k in ("curr", "status", "und"))
    _, outs, cnt = _run_track(gpu_ctx, sc, [dict(pts=pts, grid=grid, is_new=sc["is_new"], stored_desc=stored)], counters=(5, 6))
    _check_track(outs[0], ref, sc["cam"][0], (name, n, grid))
    assert cnt == (5 + ref["point_levels"], 6 + ref["iterations"]) and (n > 0 or cnt == (5, 6))


@pytest.mark.parametrize("name", ["pipe_L3_old_rot_shift", "pipe_L4_old_I_half"])
def test_track_stage_two_sets_in_one_launch(gpu_ctx, name):
    """blocks [0, grid0) the old tracks, the rest the new points (the frame path's LVK_LK_MERGED launch): each set as if launched alone"""
    sc = K.track_case(name)
    n0, grid0, n1, grid1 = 41, 50, 33, 33
    old, new = sc["pts"][:n0], sc["pts"][-n1:]
    r0 = K.track_reference(sc, old, 0, sc["stored"][:n0], grid=grid0)
    r1 = K.track_reference(sc, new, 1, None, grid=grid1)
    sets = [dict(pts=old, grid=grid0, is_new=0, stored_desc=sc["stored"][:n0]), dict(pts=new, grid=grid1, is_new=1)]
    _, outs, cnt = _run_track(gpu_ctx, sc, sets)
    _check_track(outs[0], r0, 0, "old set"); _check_track(outs[1], r1, 0, "new set")
    assert cnt == (r0["point_levels"] + r1["point_levels"], r0["iterations"] + r1["iterations"])
    for s, r in zip(sets, (r0, r1)):                          # ... and equal to their single-set launches
        _, single, _ = _run_track(gpu_ctx, sc, [s])
        _check_track(single[0], r, 0, "alone")


# =========================================================================== commit stage
@pytest.mark.parametrize("name", list(K.COMMIT_CASES))
def test_commit_stage(gpu_ctx, name):
    from larvio_amd import ops
    cc = K.commit_case(name)
    K.check_commit_case(cc)
    dst = {k: v.copy() for k, v in cc["dst"].items()}
    assert all(len(v) == cc["cap"] for v in dst.values())     # exactly cap slots: there is no slot >= cap to write
    _, state = ops.fe_commit_stage(gpu_ctx, cc["mode"], cc["cap"], cc["src"], dst, cc["state"], n=cc["n"])
    assert state == cc["ref_state"], (state, cc["ref_state"], cc["branch"])
    s = cc["branch"]["scratch"]                               # (a bootstrap that failed behind its mask: fe_frame_ref.commit_ref)
    for k in dst:
        _same(dst[k][s:], cc["ref_dst"][k][s:], f"{name}: {k}")


# =========================================================================== message stage
@pytest.mark.parametrize("name", list(K.MSG_CASES))
def test_msg_stage(gpu_ctx, name):
    from larvio_amd import ops
    mc = K.msg_case(name)
    K.check_msg_case(mc)
    n, cap = mc["n"], mc["cap"]
    ts = {k: v.copy() for k, v in mc["set"].items()}
    model, intr, dist = mc["cam"]
    _, out, state = ops.fe_msg_stage(gpu_ctx, ts, cap, n, model, intr, dist, K.MSG_DT[0], K.MSG_DT[1], mc["prev_is_last"], K.MSG_STATE, fill=FILL)
    ref = mc["ref_out"]
    assert state == mc["ref_state"]
    _same(ts["init"], mc["ref_init"], "init after the call")
    _same(out[n:], ref[n:], "slots beyond n")
    if model == 0:
        _same(out, ref, "message")
        return
    # fisheye: the undistorted float32 points a', b' are within rtol = 2e-7 of the reference's a, b (test_undistort), so a difference obeys
    # |(a' - b') - (a - b)| <= 2e-7 |a| + 2e-7 |b| <= 2 * 2e-7 * max(|a|, |b|), and the velocity that bound over dt
    g, r = out[:n], ref[:n]
    assert np.array_equal(g["id"], r["id"])
    for f in ("u", "v", "u_init", "v_init"):
        assert np.allclose(g[f], r[f], rtol=2e-7, atol=0), f
    real = r["u_init"] != -1
    assert np.array_equal(g["u_init"] != -1, real)
    prev = R.lvo.undistort(mc["set"]["ppts"][:n], intr, model, dist, R.UNIT).astype(np.float64)
    cur = np.stack([r["u"], r["v"]], 1); ini = np.stack([r["u_init"], r["v_init"]], 1)
    a = cur if mc["prev_is_last"] else prev
    for j, (f, fi) in enumerate((("u_vel", "u_init_vel"), ("v_vel", "v_init_vel"))):
        assert (np.abs(g[f] - r[f]) <= 2 * 2e-7 * np.maximum(np.abs(cur[:, j]), np.abs(prev[:, j])) / K.MSG_DT[0]).all(), f
        bound = 2 * 2e-7 * np.maximum(np.abs(a[:, j]), np.abs(ini[:, j])) / K.MSG_DT[1]
        assert (np.abs(g[fi] - r[fi])[real] <= bound[real]).all() and (g[fi][~real] == 0).all(), fi


# =========================================================================== refusals: host-side checks only, nothing is launched
ARG, CAPACITY, UNSUPPORTED = 1, 3, 4


def _filled(outs):
    return all((o[k].view(np.uint8) == FILL).all() for o in outs for k in ("curr", "status", "und", "desc") if o[k] is not None)


TRACK_REFUSALS = {
    "n_negative": (dict(n=-1), {}, ARG), "n_beyond_grid": (dict(grid=5), {}, ARG), "grid_beyond_slots": (dict(grid=R.FM_MAX_N + 1), {}, CAPACITY),
    "point_right_of_image": (dict(poke=(3, (320.0, 10.0))), {}, ARG), "point_above_image": (dict(poke=(0, (10.0, -0.25))), {}, ARG),
    "point_nan": (dict(poke=(7, (np.nan, 10.0))), {}, ARG), "point_inf": (dict(poke=(7, (10.0, np.inf))), {}, ARG),
    "pipe_with_window_15": ({}, dict(variant=2, win=15), UNSUPPORTED), "pipe_with_five_levels": ({}, dict(variant=2, levels=5, size=(640, 480)), UNSUPPORTED),
    "second_set_with_variant_1": ({}, dict(variant=1, second=True), ARG), "size_mismatch": ({}, dict(width=321), ARG), "height_mismatch": ({}, dict(height=239), ARG),
    "window_mismatch": ({}, dict(patch=15), ARG), "null_H": ({}, dict(H=None), ARG), "null_output": (dict(null_out=True), {}, ARG),
    "null_stored_desc": (dict(stored_desc=None, is_new=0), {}, ARG), "variant_3": ({}, dict(variant=3), ARG), "is_new_2": (dict(is_new=2), {}, ARG),
}


@pytest.mark.parametrize("name", list(TRACK_REFUSALS))
def test_track_stage_refusals(gpu_ctx, name):
    from larvio_amd import ops
    over_set, over, code = TRACK_REFUSALS[name]
    w, h = over.get("size", (320, 240)); win = over.get("win", 21); levels = over.get("levels", 2)
    img = K.frame_pair(320, 240, "shift")[0] if (w, h) == (320, 240) else np.tile(K.frame_pair(320, 240, "shift")[0], (2, 2))
    g = ops.Pyramid(gpu_ctx, w, h, win, levels - 1).build(img); g.orb_prepare()
    assert g.n_levels == levels
    pts = np.random.default_rng(1).uniform(5, 200, (12, 2)).astype(np.float32)
    s = dict(pts=pts, is_new=1, grid=12)
    if "poke" in over_set:
        i, p = over_set["poke"]; pts[i] = p
    s.update({k: v for k, v in over_set.items() if k != "poke"})
    sets = [s] + ([dict(pts=pts.copy(), is_new=1)] if over.get("second") else [])
    H = over["H"] if "H" in over else np.eye(3, dtype=np.float32)
    st, outs, cnt = ops.fe_track_stage(gpu_ctx, g, g, sets, over.get("patch", win), over.get("variant", 1 if win != 21 else 2), H, 0, (190.0, 190.0, 160.0, 120.0),
                                       (0.0, 0.0, 0.0, 0.0), fill=FILL, counters=(11, 12), width=over.get("width"), height=over.get("height"), check=False)
    assert st == code, (st, code)
    assert _filled(outs) and cnt == (11, 12)
    g.close()


def _commit_args(cap=64, n=30):
    cc = K.commit_case("m1_m20_appends")
    return dict(mode=1, cap=cap, n=n, src={k: (None if v is None else v.copy()) for k, v in cc["src"].items()}, state=dict(cc["state"]))


COMMIT_REFUSALS = {
    "n_negative": (dict(n=-1), ARG), "n_beyond_cap": (dict(cap=16), CAPACITY), "cap_beyond_lds": (dict(cap=R.FM_MAX_N + 1), CAPACITY),
    "cap_zero": (dict(cap=0, n=0), ARG), "mode_3": (dict(mode=3), ARG), "status_byte_4": (dict(poke_status=4), ARG), "status_byte_255": (dict(poke_status=255), ARG),
    "dst_n_negative": (dict(dst_n=-1), ARG), "dst_n_beyond_cap": (dict(dst_n=65), ARG), "n_new_is_not_n": (dict(n_new=29), ARG),
    "null_status": (dict(null="status"), ARG), "null_und": (dict(null="und"), ARG), "null_dst_life": (dict(null_dst="life"), ARG), "und_nan": (dict(poke_und=np.nan), ARG),
    "mode_0_without_ids": (dict(mode=0), ARG),
}


@pytest.mark.parametrize("name", list(COMMIT_REFUSALS))
def test_commit_stage_refusals(gpu_ctx, name):
    from larvio_amd import ops
    over, code = COMMIT_REFUSALS[name]
    a = _commit_args()
    for k in ("mode", "cap", "n"):
        a[k] = over.get(k, a[k])
    for k in ("dst_n", "n_new"):
        a["state"][k] = over.get(k, a["state"][k])
    if "poke_status" in over:
        a["src"]["status"][17] = over["poke_status"]
    if "poke_und" in over:
        a["src"]["und"][29, 1, 0] = over["poke_und"]
    if "null" in over:
        a["src"][over["null"]] = None
    slots = min(max(a["cap"], 1), 64)                         # (a cap beyond the limit is refused before any array is looked at)
    dst = ops.track_set_arrays(slots, FILL)
    if "null_dst" in over:
        dst[over["null_dst"]] = None
    st, state = ops.fe_commit_stage(gpu_ctx, a["mode"], a["cap"], a["src"], dst, a["state"], n=a["n"], check=False)
    assert st == code, (st, code)
    assert state == a["state"] and all((v.view(np.uint8) == FILL).all() for v in dst.values() if v is not None)


MSG_REFUSALS = {"n_negative": (dict(n=-1), ARG), "n_beyond_cap": (dict(n=9), CAPACITY), "cap_beyond_slots": (dict(cap=R.FM_MAX_N + 1), CAPACITY), "cap_zero": (dict(cap=0, n=0), ARG),
                "null_init": (dict(null="init"), ARG), "prev_is_last_2": (dict(prev_is_last=2), ARG), "dt_nan": (dict(dt_1=np.nan), ARG), "model_2": (dict(model=2), ARG)}


@pytest.mark.parametrize("name", list(MSG_REFUSALS))
def test_msg_stage_refusals(gpu_ctx, name):
    from larvio_amd import ops
    over, code = MSG_REFUSALS[name]
    ts = {k: v[:8].copy() for k, v in K.msg_case("n65_last0_radtan")["set"].items()}
    before = {k: v.copy() for k, v in ts.items()}
    if "null" in over:
        ts[over["null"]] = None
    st, out, state = ops.fe_msg_stage(gpu_ctx, ts, over.get("cap", 8), over.get("n", 5), over.get("model", 0), (190.0, 190.0, 160.0, 120.0), (0.0, 0.0, 0.0, 0.0),
                                      over.get("dt_1", 0.05), 0.1, over.get("prev_is_last", 0), K.MSG_STATE, fill=FILL, check=False)
    assert st == code, (st, code)
    assert (out.view(np.uint8) == FILL).all() and state == K.MSG_STATE and all(np.array_equal(_bits(v), _bits(before[k])) for k, v in ts.items() if v is not None)
