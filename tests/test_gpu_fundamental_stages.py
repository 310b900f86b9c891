"""fm_mask_block (larvio_amd/csrc/fe_track_dev.h), the device form of cv::findFundamentalMat(FM_RANSAC), off its fast path: every case of
tests/fm_cases.py through the stage entries it names (lvk_ransac_fundamental, lvk_find_fundamental_mask, lvk_find_fundamental), one
single-workgroup launch each, against the sequential C oracle (oracle/lvo.py).  Masks and iteration counts identical, F bit for bit
(one set is a strict expected failure there: F_LAST_PLACE below).
Output buffers are pre-filled (mask 0xA5, info -7, F NaN) and the mask buffer is 64 bytes longer than n: what a call does not write keeps its fill.
tests/test_fm_cases.py proves, without a GPU, that each case reaches the path it is listed for.

    path                                                          case(s)
    table overrun (pos + 256 > 4096: sequential draw from        overrun_n60 (256 threads), overrun_n600 (512 threads); also cap_n40,
      FM_RNG.s[pos - 1] for the rest of the call)                   nothing_found_n30, collinear_round0_n40 behind their first event
    collinear subset in the fast path (sh_anybad, whole round     collinear_round0_n40 (hypothesis 1, round 0), collinear_late_n40
      redrawn sequentially from pos)                                (hypothesis 14, round 2), repeated_n30 (a repeated point is collinear)
    subset does not fit the 256-draw window (FM_NOFIT / o >= 256) misfit_n8_far (round 9, hypothesis 135).  misfit_n8 / n9 / n10, the noisy
                                                                    two-view sets where it looks likely, cannot reach it: the draws depend on n
                                                                    alone, the first misfit for n = 8 is at hypothesis 135 and 8 points stop
                                                                    after at most 9; for n = 9, 10 the table ends first (fm_cases.MISFIT)
    getSubset fails at iteration 0 (no model, zero mask)          all_collinear_n20
    getSubset fails at a later iteration (keep the best so far)   no input constructed: it needs 10000 collinear attempts in a row behind a
                                                                    hypothesis that was not collinear, on the same points
    no model with more than 6 inliers at the cap (sh_ctl[1] == 0) nothing_found_n30, misfit_n8_far: coordinates near 1e8, where a model
                                                                    misses its own sample by more than 0.05 px.  In the image range every model
                                                                    counts its own seven points (cap_sample_only_n30: uniform pairs in the image, mask not 0)
    iteration cap (1000 without the bound collapsing)             cap_n40, cap_sample_only_n30
    max_iters inside round 0 / round 1 / at their edges           max_iters_0, 1, 2, 3, 7, 8, 9, 24, 25
    d_nullspace_7x9 zero column norm, d_solve_cubic a0 == 0 /     frozen_n15, frozen_n60, shift_n60, rotation_n60, planar_n60,
      d == 0 / one real root, d_7pt_finish |s| <= eps               planar_noisy_n60, repeated_n30, grid_n49, lmeds_frozen_n8 / n14;
                                                                    the solver alone: cubic_0, cubic_1, cubic_2, cubic_3 (n = 7)
    LMedS on exact data (median 0, sigma at its floor)            lmeds_exact_n8 / n11 / n14, lmeds_frozen_n8 / n14
    width and capacity edges of the entries                       width_n511 / n512 / n513, capacity_n4096, test_capacity_refusal
    defaults (thresh <= 0 -> 3, conf outside (eps, 1 - eps))      default_thresh_0 / thresh_neg / conf_0 / conf_1

"No model": the kernel and the oracle agree - a zero mask, F all zeros (OpenCV's empty Mat), d_info[0] = 1 (the mask was written: the
reference's callers read it and drop every point, image_processor.cpp:498, 755, 968) and d_info[1] the hypotheses drawn (0 when the first
getSubset failed, 1000 at the cap).  Neither side needed a change."""
import ctypes as C
import numpy as np
import pytest
from tests import fm_cases as K

pytestmark = pytest.mark.gpu
FILL, PAD = K.FILL, 64
ARG, CAPACITY = 1, 3
ENTRY = dict(ransac="lvk_ransac_fundamental", mask="lvk_find_fundamental_mask", F="lvk_find_fundamental")


def _call(ctx, entry, p1, p2, thresh=1.0, conf=0.99, max_iters=1000, n=None, null=()):
    """one call with pre-filled outputs -> (status, mask bytes (n + PAD), info (2,), F (9,))"""
    from larvio_amd._lib import lib, _p
    n = len(p1) if n is None else n
    slots = min(max(n, 0), K.FM_MAX_N + 1)
    da, db = ctx.to_device(np.ascontiguousarray(p1, np.float32)), ctx.to_device(np.ascontiguousarray(p2, np.float32))
    dm = ctx.to_device(np.full(slots + PAD, FILL, np.uint8)); di = ctx.to_device(np.full(2, -7, np.int32)); dF = ctx.to_device(np.full(9, np.nan))
    a = [ctx.h, None if "p1" in null else _p(da), None if "p2" in null else _p(db), n, thresh, conf]
    if entry == "ransac":
        a.append(max_iters)
    a += [None if "mask" in null else _p(dm), _p(di)]
    if entry == "F":
        a.append(None if "F" in null else _p(dF))
    st = getattr(lib(), ENTRY[entry])(*a)
    ctx.sync()
    return st, ctx.to_host(dm, np.uint8, (slots + PAD,)), ctx.to_host(di, np.int32, (2,)), ctx.to_host(dF, np.float64, (9,))


def _untouched(mask, info, F):
    return (mask == FILL).all() and (info == -7).all() and np.isnan(F).all()


def _bits(F):
    return np.ascontiguousarray(F, np.float64).reshape(-1).view(np.uint64)


def _cases(entry):
    return [name for name, c in K.CASES.items() if entry in c["entries"]]


def _check_find(c, o, entry, mask, info, F, bits=True):
    n = c["n"]
    mo, Fo = o["find"]
    assert (mask[n:] == FILL).all(), "bytes behind the mask"
    assert mo is not None and info[0] == 1
    assert np.array_equal(mask[:n], mo), (int(mask[:n].sum()), int(mo.sum()))
    if n >= 15:
        assert info[1] == o["ransac"][2], (info[1], o["ransac"][2])
    if entry == "F":
        assert not np.isnan(F).any() and F.any() == Fo.any()
        if bits:
            assert np.array_equal(_bits(F), _bits(Fo)), (F, Fo.ravel())
    else:
        assert np.isnan(F).all()


@pytest.mark.parametrize("name", _cases("ransac"))
def test_ransac_entry(gpu_ctx, name):
    c, o = K.case(name), K.oracle(name)
    ok, mo, ito = o["ransac"]
    st, mask, info, F = _call(gpu_ctx, "ransac", c["p1"], c["p2"], c["thresh"], c["conf"], c["max_iters"])
    assert st == 0
    print(name, "iterations", info[1], "oracle", ito, "inliers", int(mask[:c["n"]].sum()), "oracle", int(mo.sum()))
    assert info[0] == 1 and info[1] == ito, (info, ito)
    assert np.array_equal(mask[:c["n"]], mo), (int(mask[:c["n"]].sum()), int(mo.sum()))
    assert ok or not mask[:c["n"]].any()
    assert (mask[c["n"]:] == FILL).all() and np.isnan(F).all()


@pytest.mark.parametrize("name", _cases("mask"))
def test_mask_entry(gpu_ctx, name):
    c, o = K.case(name), K.oracle(name)
    st, mask, info, F = _call(gpu_ctx, "mask", c["p1"], c["p2"], c["thresh"], c["conf"])
    assert st == 0
    _check_find(c, o, "mask", mask, info, F)


_F_RUNS = {}


def _matrix_run(ctx, name):
    if name not in _F_RUNS:                                   # one launch serves the two tests below
        c = K.case(name)
        _F_RUNS[name] = _call(ctx, "F", c["p1"], c["p2"], c["thresh"], c["conf"])
    return _F_RUNS[name]


@pytest.mark.parametrize("name", _cases("F"))
def test_matrix_entry(gpu_ctx, name):
    """mask, iteration count, the bytes behind the mask, and F zero exactly when the oracle's is"""
    st, mask, info, F = _matrix_run(gpu_ctx, name)
    assert st == 0
    _check_find(K.case(name), K.oracle(name), "F", mask, info, F, bits=False)


# Sets on which F agrees with the oracle's except in the last places of some entries (mask and iterations identical): the winning model's
# root of the cubic went through d_solve_cubic's acos / cos / pow, which the device's and the host's math libraries round differently.
# Observed on lmeds_frozen_n8: entries 0, 4, 5 and 7 differ by 6 to 8 units in the last place, the others not at all (PARITY.md); the winner
# is hypothesis 238, the only model of its subset, so the root came from the one-real-root branch: pow(d + |R|, 1. / 3).  The cure
# is one restated routine compiled on both sides, as lvk_sincosf.h is for cosf / sinf; until then the comparison stays exact and is
# expected to fail, strictly, on exactly these.
F_LAST_PLACE = {"lmeds_frozen_n8"}


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.xfail(strict=True, reason="cubic root through acos/cos/pow: libm and ocml differ in the last place"))
                                  if n in F_LAST_PLACE else n for n in _cases("F")])
def test_matrix_entry_bits(gpu_ctx, name):
    """F bit for bit (the contract test_find_fundamental_returns_the_registrators_model states)"""
    st, mask, info, F = _matrix_run(gpu_ctx, name)
    assert st == 0 and np.array_equal(_bits(F), _bits(K.oracle(name)["find"][1])), (F, K.oracle(name)["find"][1].ravel())


@pytest.mark.parametrize("n", range(7))
def test_below_the_minimum_nothing_is_written(gpu_ctx, n):
    from oracle import lvo
    c = K.case("easy_n60")
    p1, p2 = c["p1"][:n], c["p2"][:n]
    mo, Fo = lvo.find_fundamental(p1, p2)
    assert mo is None and not Fo.any()
    for entry in ("mask", "F"):
        st, mask, info, F = _call(gpu_ctx, entry, p1, p2)
        assert st == 0 and (mask == FILL).all() and tuple(info) == (0, 0)
        assert (_bits(F) == 0).all() if entry == "F" else np.isnan(F).all()


def test_ransac_entry_refuses_seven_points(gpu_ctx):
    from larvio_amd._lib import lib
    c = K.case("easy_n60")
    st, mask, info, F = _call(gpu_ctx, "ransac", c["p1"][:7], c["p2"][:7])
    assert st == ARG and "lvk_ransac_fundamental" in lib().lvk_last_error(gpu_ctx.h).decode()
    assert _untouched(mask, info, F)


@pytest.mark.parametrize("entry", list(ENTRY))
def test_capacity_refusal(gpu_ctx, entry):
    """n = FM_MAX_N + 1 is refused with nothing written, and the context goes on working: the next call still matches the oracle"""
    big = K.case("capacity_n4096")
    p1 = np.concatenate([big["p1"], big["p1"][:1]]); p2 = np.concatenate([big["p2"], big["p2"][:1]])
    st, mask, info, F = _call(gpu_ctx, entry, p1, p2)
    assert st == CAPACITY and _untouched(mask, info, F)
    c, o = K.case("easy_n60"), K.oracle("easy_n60")
    st, mask, info, F = _call(gpu_ctx, entry, c["p1"], c["p2"])
    assert st == 0 and info[1] == o["ransac"][2] and np.array_equal(mask[:c["n"]], o["ransac"][1]) and (mask[c["n"]:] == FILL).all()


@pytest.mark.parametrize("entry,null", [(e, k) for e in ENTRY for k in ("p1", "p2", "mask")] + [("F", "F")])
def test_null_pointer_refusals(gpu_ctx, entry, null):
    c = K.case("easy_n60")
    st, mask, info, F = _call(gpu_ctx, entry, c["p1"], c["p2"], null=(null,))
    assert st == ARG and _untouched(mask, info, F)


def test_no_state_survives_a_call(gpu_ctx):
    """one context, one stream, in order: a table overrun (ends on the sequential path), the all-collinear set (ends without a model), an easy set
    (must start on the table path again, with a fresh generator and no best model), the overrun again, then LMedS - each equal to the
    oracle, the two overrun runs identical.  sh_serial, sh_rng, sh_pos or sh_ctl surviving a call would show in the call behind it."""
    runs = []
    for name in ("overrun_n60", "all_collinear_n20", "easy_n60", "overrun_n60", "lmeds_exact_n11"):
        c, o = K.case(name), K.oracle(name)
        st, mask, info, F = _call(gpu_ctx, "F", c["p1"], c["p2"], c["thresh"], c["conf"])
        assert st == 0, name
        _check_find(c, o, "F", mask, info, F)
        runs.append((mask, info, F))
    for a, b in zip(runs[0], runs[3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
