"""lvk_ekf_update_sparse (k_fix_gain, k_fix_downdate, be_fix.hip) against the long-double restatement tests/fix_ref.py, inside the
componentwise bound derived there: n = 28, 34, 63, 64, 65 and 433, ldp = n and padded, m = 3 and 6, ncols 3, 6 and 12 with the first three
and the last six columns of P, a in {0, 0.5, 1}, zero and non-zero lever arm (fix_ref.stage_problems); exact symmetry; repeatability;
NaN in everything the call must not read; a gated and an indefinite case that leave every byte of P; every refusal."""
import numpy as np
import pytest

from tests import fix_ref as F

pytestmark = pytest.mark.gpu
LD = F.LD


def _run(ctx, pr, **kw):
    from larvio_amd import ops
    return ops.update_sparse(ctx, F.buffer(pr["P"], pr["n"], pr["ldp"]), F.record(pr, **kw), n=pr["n"])


@pytest.fixture(scope="module")
def problems():
    """every problem with its reference, computed once"""
    return [(pr, F.update_tracked(pr["P"], pr["cols"], pr["H"], pr["r"], pr["R"], pr["gate"])) for pr in F.stage_problems()]


@pytest.fixture(scope="module")
def results(gpu_ctx, problems):
    return [_run(gpu_ctx, pr) for pr, _ in problems]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_stage_entry_against_the_restatement_within_the_derived_bound(problems, results):
    worst = {}
    for (pr, t), (dx, Pb, info) in zip(problems, results):
        n = pr["n"]
        assert int(info[0]) == t["status"] and info[3] == 0, pr["name"]
        assert np.all(np.isfinite(dx)) and np.all(np.isfinite(Pb[:, :n])) and np.all(np.isnan(Pb[:, n:]))
        wg = abs(LD(info[1]) - t["gamma"]) / t["e_gamma"]
        assert abs(LD(info[2]) - t["pmin"]) <= 1e-6 * abs(t["pmin"])
        if t["status"] == 0:
            wd = F.worst_ratio(dx.astype(LD) - t["dx"], t["e_dx"]); wp = F.worst_ratio(Pb[:, :n].astype(LD) - t["P"], t["e_P"])
        else:
            assert np.all(dx == 0) and _same_bits(Pb, F.buffer(pr["P"], n, pr["ldp"]))
            wd = wp = 0.0
        print("%-20s n %3d ldp %3d m %d ncols %2d status %d: worst |error| / bound dx %.3f P %.3f gamma %.3f" %
              (pr["name"], n, pr["ldp"], pr["H"].shape[0], pr["H"].shape[1], t["status"], wd, wp, float(wg)))
        key = "n <= 65" if n <= 65 else "n = 433"
        worst[key] = max(worst.get(key, 0.0), wd, wp, float(wg))
    print("worst |error| / bound per group:", worst)
    assert max(worst.values()) <= 1.0


def test_P_is_exactly_symmetric_and_two_calls_give_the_same_bits(gpu_ctx, problems, results):
    for (pr, _), (dx, Pb, info) in zip(problems, results):
        n = pr["n"]
        assert _same_bits(pr["P"], pr["P"].T)
        assert _same_bits(Pb[:, :n], Pb[:, :n].T), pr["name"]
        dx2, Pb2, info2 = _run(gpu_ctx, pr)
        assert _same_bits(dx, dx2) and _same_bits(info, info2) and np.array_equal(Pb.view(np.uint64), Pb2.view(np.uint64))


def test_nan_in_everything_the_call_must_not_read_changes_nothing(gpu_ctx, problems, results):
    """NaN in every entry of H and cols beyond ncols, of r beyond m and of R beyond m x m (cols: -1); the padding of P is NaN throughout"""
    for (pr, _), (dx, Pb, info) in zip(problems, results):
        rec = F.record(pr, fill=np.nan)
        m, nc = pr["H"].shape
        assert np.all(np.isnan(rec["H"][0, m * nc:])) and np.all(np.isnan(rec["R"][0, m * m:])) and np.all(rec["cols"][0, nc:] == -1)
        dx2, Pb2, info2 = _run(gpu_ctx, pr, fill=np.nan)
        assert _same_bits(dx, dx2) and _same_bits(info, info2) and np.array_equal(Pb.view(np.uint64), Pb2.view(np.uint64)), pr["name"]
        # the lower triangle of R is not read either
        R = pr["R"].copy(); R[np.tril_indices(m, -1)] = 1e300
        dx3, Pb3, _ = _run(gpu_ctx, pr, R=R)
        assert _same_bits(dx, dx3) and np.array_equal(Pb.view(np.uint64), Pb3.view(np.uint64))


def test_gated_and_indefinite_cases_leave_every_byte_of_P(gpu_ctx, problems, results):
    n_gated = 0
    for (pr, t), (dx, Pb, info) in zip(problems, results):
        before = F.buffer(pr["P"], pr["n"], pr["ldp"])
        if t["status"] == 1:
            assert int(info[0]) == 1 and np.all(dx == 0) and before.tobytes() == Pb.tobytes()
            n_gated += 1
        # R made indefinite through the stage entry: S = H P_s H^T + R loses a pivot
        m = pr["H"].shape[0]
        S = F.update(pr["P"], pr["cols"], pr["H"], pr["r"], pr["R"])["S"].astype(np.float64)
        R = pr["R"] - 2 * np.diag(np.diag(S))
        dx2, Pb2, info2 = _run(gpu_ctx, pr, R=R, gate=0.0)
        assert int(info2[0]) == 2 and info2[1] == 0 and not info2[2] > 0, (pr["name"], info2)
        assert np.all(dx2 == 0) and before.tobytes() == Pb2.tobytes()
    assert n_gated == 2


def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx, problems, results):
    import ctypes as C
    from larvio_amd._lib import lib, _p
    k = 3                                                                    # n = 34, padded, twelve columns
    pr, _ = problems[k]; good = results[k]
    n = pr["n"]; rec = F.record(pr)
    Lb = lib(); dP = gpu_ctx.to_device(F.buffer(pr["P"], n, pr["ldp"]))
    dx = np.full(n, 7.0); info = np.full(4, 7.0)
    vp, i = C.c_void_p, C.c_int
    Lb.lvk_ekf_update_sparse.argtypes = [vp, vp, i, i, vp, vp, vp]; Lb.lvk_ekf_update_sparse.restype = i

    def call(d_P=dP, ld=pr["ldp"], nn=n, u=rec, h_dx=dx, h_info=info, ctx=gpu_ctx.h):
        ptr = lambda a: None if a is None else _p(a)
        return Lb.lvk_ekf_update_sparse(ctx, ptr(d_P), ld, nn, ptr(u), ptr(h_dx), ptr(h_info))

    def rec_with(**kw):
        u = rec.copy()
        for key, (idx, v) in kw.items():
            if idx is None:
                u[key] = v
            else:
                u[key][0, idx] = v
        return u
    bad = [dict(d_P=None), dict(u=None), dict(h_dx=None), dict(h_info=None), dict(ld=n - 1), dict(nn=0),
           dict(u=rec_with(m=(None, 4))), dict(u=rec_with(m=(None, 0))), dict(u=rec_with(ncols=(None, 0))), dict(u=rec_with(ncols=(None, 13))),
           dict(u=rec_with(cols=(0, -1))), dict(u=rec_with(cols=(11, n))), dict(u=rec_with(cols=(5, rec["cols"][0, 4]))), dict(u=rec_with(cols=(5, rec["cols"][0, 3]))),
           dict(u=rec_with(H=(7, np.nan))), dict(u=rec_with(H=(35, np.inf))), dict(u=rec_with(r=(2, np.nan))), dict(u=rec_with(R=(4, -np.inf))),
           dict(u=rec_with(gate=(None, np.nan)))]
    for kw in bad:
        assert call(**kw) == 1, kw                                    # LVK_ERR_ARG
        assert np.all(dx == 7.0) and np.all(info == 7.0)              # nothing written
        assert b"lvk_ekf_update_sparse" in Lb.lvk_last_error(gpu_ctx.h)
    assert call(ctx=None) == 1 and np.all(dx == 7.0)
    assert gpu_ctx.to_host(dP, np.float64, (n, pr["ldp"])).tobytes() == F.buffer(pr["P"], n, pr["ldp"]).tobytes()      # P untouched by all of them
    assert call() == 0                                                 # ... and the context is usable
    assert np.array_equal(dx.view(np.uint64), good[0].view(np.uint64)) and np.array_equal(info.view(np.uint64), good[2].view(np.uint64))
    assert np.array_equal(gpu_ctx.to_host(dP, np.float64, (n, pr["ldp"])).view(np.uint64), good[1].view(np.uint64))
