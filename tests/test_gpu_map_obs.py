"""lvk_map_gather_obs (larvio_amd/csrc/fe_mapobs.hip) as a stage: bit for bit against a numpy restatement that follows include/lvk_c.h
expression by expression, at the sizes where the compaction changes shape (one lane, a wavefront's edge, every wavefront), with every
status mixed in, with indices outside the map, twice over for determinism, and against larvio_amd.localize.map_obs.

map_obs has no fixed order for the covariance (Rz @ cov @ Rz.T through numpy's matmul); its p_w must agree bit for bit, its cov_w to a
relative bound.  The bound: the float64 matmul form against the same product in long double, on the very covariances of the test, differs
by at most 2.0e-16 of the largest entry of a matrix (measured in the test itself, which prints it); the stage entry is held to ten times the
value measured in the run."""
import numpy as np
import pytest

from larvio_amd import localize
from larvio_amd._lib import MAP_MATCH, MATCH_OK

pytestmark = pytest.mark.gpu
N_MAP = 300
SIZES = (0, 1, 63, 64, 65, 1024)
C_, S_ = np.cos(0.7), np.sin(0.7)
ALIGN = (C_, S_, np.array([3.0, -2.0, 0.5]))


def restate(rec, X, cov, align, sigma):
    """the header's expressions in the header's order -> (obs, idx, n_ok, n_bad)"""
    from larvio_amd.ops import LANDMARK_OBS
    c, s, t = (np.float64(1.0), np.float64(0.0), np.zeros(3)) if align is None else (np.float64(align[0]), np.float64(align[1]), np.asarray(align[2], np.float64))
    n_map = len(X)
    okst = rec["m"]["status"] == MATCH_OK
    inside = (rec["index"] >= 0) & (rec["index"] < n_map)
    idx = np.nonzero(okst & inside)[0].astype(np.int32)
    k = rec["index"][idx]
    obs = np.zeros(len(idx), LANDMARK_OBS)
    x0, x1, x2 = X[k, 0], X[k, 1], X[k, 2]
    q0 = c * x0 - s * x1; q1 = s * x0 + c * x1
    obs["p_w"][:, 0] = q0 + t[0]; obs["p_w"][:, 1] = q1 + t[1]; obs["p_w"][:, 2] = x2 + t[2]
    if cov is not None:
        S = cov.reshape(-1, 9)[k]
        a, b, d, e, f, g = S[:, 0], S[:, 1], S[:, 4], S[:, 2], S[:, 5], S[:, 8]
        m00 = c * a - s * b; m01 = c * b - s * d; m10 = s * a + c * b; m11 = s * b + c * d
        w00 = m00 * c - m01 * s; w01 = m00 * s + m01 * c; w11 = m10 * s + m11 * c
        w02 = c * e - s * f; w12 = s * e + c * f
        obs["cov_w"] = np.stack([w00, w01, w02, w01, w11, w12, w02, w12, g], -1)
    obs["uv"] = rec["m"]["und"][idx].astype(np.float64)
    obs["sigma"] = sigma
    return obs, idx, len(idx), int((okst & ~inside).sum())


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(5)
    X = rng.uniform(-20, 20, (N_MAP, 3))
    B = rng.normal(0, 0.05, (N_MAP, 3, 3))
    cov = B @ B.transpose(0, 2, 1) + 1e-4 * np.eye(3)
    cov = np.triu(cov) + np.triu(cov, 1).transpose(0, 2, 1)
    return X, cov


def records(n, seed, status="mixed", n_map=N_MAP):
    rng = np.random.default_rng(seed)
    rec = np.zeros(n, MAP_MATCH)
    rec["index"] = rng.integers(0, n_map, n)
    rec["cell"] = rng.integers(0, 20, n)
    rec["m"]["status"] = {"mixed": rng.integers(0, 5, n), "none": rng.integers(1, 5, n), "all": np.zeros(n, np.int64)}[status]
    rec["m"]["dist"] = rng.integers(0, 58, n)
    rec["m"]["und"] = rng.uniform(-0.6, 0.6, (n, 2)).astype(np.float32)
    rec["m"]["px"] = rng.uniform(0, 700, (n, 2)).astype(np.float32)
    rec["q"]["x"] = rng.uniform(0, 700, n); rec["q"]["radius"] = 12
    return rec


def _check(gpu_ctx, rec, X, cov, align, sigma=0.002):
    from larvio_amd import ops
    out = ops.map_gather_obs(gpu_ctx, rec, X, cov, sigma, align=align)
    obs, idx, n_ok, n_bad = restate(rec, X, cov, align, sigma)
    assert int(out["info"]["n_ok"]) == n_ok and int(out["info"]["n_bad"]) == n_bad and not out["info"]["pad"].any()
    assert np.array_equal(out["idx"], idx)
    assert out["obs"].tobytes() == obs.tobytes()
    G = ops.MAP_OBS_GUARD
    for k, item in (("obs", obs.dtype.itemsize), ("idx", 4)):                      # nothing beyond n_ok entries, nothing in the guards
        raw = out[k + "_raw"]
        assert (raw[:G] == 0xA5).all() and (raw[G + n_ok * item:] == 0xA5).all(), k
    assert (out["info_raw"][:G] == 0xA5).all() and (out["info_raw"][G + 16:] == 0xA5).all()
    return out


@pytest.mark.parametrize("n_rec", SIZES)
def test_sizes_mixed_statuses(gpu_ctx, world, n_rec):
    """all five statuses mixed, a yawed and shifted map, at every size where the compaction changes shape"""
    X, cov = world
    out = _check(gpu_ctx, records(n_rec, 100 + n_rec), X, cov, ALIGN)
    if n_rec >= 63:
        assert 0 < int(out["info"]["n_ok"]) < n_rec


@pytest.mark.parametrize("status", ["none", "all"])
def test_none_ok_all_ok(gpu_ctx, world, status):
    X, cov = world
    for n_rec in (65, 1024):
        out = _check(gpu_ctx, records(n_rec, 7, status), X, cov, ALIGN)
        assert int(out["info"]["n_ok"]) == (0 if status == "none" else n_rec)


def test_no_covariance_and_identity(gpu_ctx, world):
    """d_cov NULL: zero covariances; align NULL and an explicit identity record: the same bytes"""
    from larvio_amd import ops
    X, cov = world
    rec = records(200, 9)
    out = _check(gpu_ctx, rec, X, None, ALIGN)
    assert not out["obs"]["cov_w"].any()
    a = _check(gpu_ctx, rec, X, cov, None)
    b = ops.map_gather_obs(gpu_ctx, rec, X, cov, 0.002, align=(1.0, 0.0, np.zeros(3)))
    assert a["obs_raw"].tobytes() == b["obs_raw"].tobytes() and a["idx_raw"].tobytes() == b["idx_raw"].tobytes() and a["info_raw"].tobytes() == b["info_raw"].tobytes()
    k = rec["index"][a["idx"]]
    assert np.array_equal(a["obs"]["p_w"], X[k])                                   # the identity moves nothing
    assert np.array_equal(a["obs"]["cov_w"].reshape(-1, 3, 3), cov[k])


def test_bad_index_is_counted_not_followed(gpu_ctx, world):
    """OK records with index -1, n_map, and far outside: counted in n_bad, not emitted; a bad index on a record that is not OK is not
    counted.  Checked by value: the emitted rows are exactly the restatement's."""
    X, cov = world
    rec = records(130, 13, "all")
    rec["index"][3] = -1; rec["index"][64] = N_MAP; rec["index"][129] = 2 ** 31 - 1; rec["index"][70] = -(2 ** 31)
    rec["m"]["status"][10] = 2; rec["index"][10] = N_MAP + 5
    out = _check(gpu_ctx, rec, X, cov, ALIGN)
    assert int(out["info"]["n_bad"]) == 4 and int(out["info"]["n_ok"]) == 130 - 5
    assert not np.isin([3, 10, 64, 70, 129], out["idx"]).any()
    out = _check(gpu_ctx, rec, X[:0], None, ALIGN)                                 # an empty map: every OK record is bad, X is not needed
    assert int(out["info"]["n_ok"]) == 0 and int(out["info"]["n_bad"]) == 129


def test_deterministic(gpu_ctx, world):
    from larvio_amd import ops
    X, cov = world
    rec = records(1024, 21)
    a = ops.map_gather_obs(gpu_ctx, rec, X, cov, 0.002, align=ALIGN)
    b = ops.map_gather_obs(gpu_ctx, rec, X, cov, 0.002, align=ALIGN)
    for k in ("obs_raw", "idx_raw", "info_raw"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_against_localize_map_obs(gpu_ctx, world):
    """p_w bit for bit; cov_w within ten times what numpy's own Rz @ cov @ Rz.T shows against long double on the same matrices"""
    from larvio_amd import ops
    from larvio_amd._lib import ALIGN_RESULT
    X, cov = world
    rec = records(1024, 33)
    res = np.zeros(1, ALIGN_RESULT); res["c"], res["s"], res["t"] = ALIGN
    cfg = dict(intrinsics=(458.654, 457.296, 367.215, 248.375))
    sigma_px = 1.5
    sigma = sigma_px / ((cfg["intrinsics"][0] + cfg["intrinsics"][1]) / 2)
    out = ops.map_gather_obs(gpu_ctx, rec, X, cov, sigma, align=res[0])
    obs, idx = localize.map_obs(rec, X, cov, res[0], sigma_px, cfg)
    assert np.array_equal(out["idx"], idx)
    assert np.array_equal(out["obs"]["uv"], obs["uv"]) and np.array_equal(out["obs"]["sigma"], obs["sigma"])
    LD = np.longdouble
    Rz = np.array([[C_, -S_, 0.0], [S_, C_, 0.0], [0.0, 0.0, 1.0]])
    k = rec["index"][idx]
    exact = Rz.astype(LD) @ cov[k].astype(LD) @ Rz.T.astype(LD)
    scale = np.abs(exact).max(axis=(1, 2))
    host = float((np.abs(obs["cov_w"].reshape(-1, 3, 3) - exact).max(axis=(1, 2)) / scale).max())
    dev = float((np.abs(out["obs"]["cov_w"].reshape(-1, 3, 3) - exact).max(axis=(1, 2)) / scale).max())
    print(f"cov_w vs long double: map_obs {host:.3e}, device {dev:.3e}")
    assert dev <= 10 * host
    assert float((np.abs(out["obs"]["cov_w"] - obs["cov_w"]).reshape(-1, 3, 3).max(axis=(1, 2)) / scale).max()) <= 11 * host
    pw_equal = np.array_equal(out["obs"]["p_w"], obs["p_w"])
    print("p_w bit for bit:", pw_equal, "max |diff|", float(np.abs(out["obs"]["p_w"] - obs["p_w"]).max()))
    assert pw_equal


def test_refusals(gpu_ctx, world):
    from larvio_amd import ops
    from larvio_amd._lib import lib, _p, MAP_OBS_INFO
    X, cov = world
    rec = records(10, 1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        st, _ = ops.map_gather_obs(gpu_ctx, rec, X, cov, bad, align=ALIGN, check=False); assert st == 1
    for al in ((np.nan, 0.0, np.zeros(3)), (1.0, np.inf, np.zeros(3)), (1.0, 0.0, np.array([0.0, np.nan, 0.0]))):
        st, _ = ops.map_gather_obs(gpu_ctx, rec, X, cov, 0.002, align=al, check=False); assert st == 1
    st, _ = ops.map_gather_obs(gpu_ctx, rec, X, cov, 0.002, n_rec=-1, check=False); assert st == 1
    big = records(1025, 2)
    st, out = ops.map_gather_obs(gpu_ctx, big, X, cov, 0.002, check=False); assert st == 3
    assert (out["obs_raw"] == 0xA5).all() and (out["info_raw"] == 0xA5).all()
    L = lib()
    d_rec = gpu_ctx.to_device(rec); d_X = gpu_ctx.to_device(X); d_obs = gpu_ctx.alloc(136 * 10); d_idx = gpu_ctx.alloc(40); d_info = gpu_ctx.alloc(16)
    args = [gpu_ctx.h, _p(d_rec), 10, _p(d_X), None, N_MAP, None, 0.002, _p(d_obs), _p(d_idx), _p(d_info)]
    for k in (1, 3, 8, 9, 10):
        a = list(args); a[k] = None
        assert L.lvk_map_gather_obs(*a) == 1, k
    a = list(args); a[5] = -1
    assert L.lvk_map_gather_obs(*a) == 1
    assert b"lvk_map_gather_obs" in L.lvk_last_error(gpu_ctx.h)
    assert L.lvk_map_gather_obs(*args) == 0                                       # the context goes on
    info = gpu_ctx.to_host(d_info, MAP_OBS_INFO, (1,))[0]
    assert int(info["n_ok"]) == int((rec["m"]["status"] == MATCH_OK).sum())
