"""Plain numpy restatement of the exchange step of the sharded update (test infrastructure): the wire layout of one rank's block and
the receiver's rules, as include/lvk_c.h states them next to lvk_shard_pack_stage.  Nothing here computes: doubles travel as their
64-bit patterns and results as their 32 bytes, so a comparison with the kernels is a comparison of bits.

  block of one rank (bytes_per_rank bytes):
    [0, 256)                      header, 16 bytes defined: u32 magic, i32 rank, i32 k, i32 n_res
    [256, 256 + res_bytes)        n_res results of 32 bytes
    [256 + res_bytes, ...)        k rows of ncols + 1 doubles, the residual last
  a block is good iff magic, rank, k, n_res equal what the receiver's meta {job_lo, job_n, k, row_off} expects of that rank;
  a bad block: its k rows and residuals become zero, its results are not copied, bit min(g, 31) of the peer-failure word is set;
  everything else in H, r and the result arrays is left alone."""
import numpy as np

HDR = 256
MAGIC = 0x4c564b58
RESULT = np.dtype([("gamma", np.float64), ("h2", np.float64), ("rows", np.int32), ("first_row", np.int32), ("c", np.int32), ("accept", np.int32)])
META = np.dtype([("job_lo", np.int32), ("job_n", np.int32), ("k", np.int32), ("row_off", np.int32)])
assert RESULT.itemsize == 32 and META.itemsize == 16


def block_bytes(res_bytes, k_max, ncols):
    """the smallest bytes_per_rank the layout needs"""
    return HDR + res_bytes + 8 * k_max * (ncols + 1)


def res_bytes_for(n_res_max):
    """the result area as the filter sizes it: the largest job count of any rank, rounded up to 256 bytes"""
    return (32 * n_res_max + 255) & ~255


def header(rank, k, n_res, magic=MAGIC):
    """the 16 defined header bytes"""
    return np.concatenate([np.array([magic], np.uint32).view(np.uint8), np.array([rank, k, n_res], np.int32).view(np.uint8)])


def pack(rank, X, rX, res, res_bytes, bytes_per_rank, fill):
    """X: k x ncols doubles, rX: k, res: n_res RESULT records -> the block (uint8); undefined bytes hold `fill`"""
    X = np.ascontiguousarray(X, np.float64); rX = np.ascontiguousarray(rX, np.float64); res = np.ascontiguousarray(res, RESULT)
    k, ncols = X.shape
    assert len(rX) == k and res_bytes % 256 == 0 and res.nbytes <= res_bytes and bytes_per_rank >= block_bytes(res_bytes, k, ncols)
    out = np.full(bytes_per_rank, fill & 0xFF, np.uint8)
    out[:16] = header(rank, k, len(res))
    out[HDR:HDR + res.nbytes] = res.view(np.uint8).reshape(-1)
    rows = np.empty((k, ncols + 1), np.uint64)
    rows[:, :ncols] = X.view(np.uint64); rows[:, ncols] = rX.view(np.uint64)
    o = HDR + res_bytes
    out[o:o + rows.nbytes] = rows.view(np.uint8).reshape(-1)
    return out


def block_is_good(block, g, meta):
    h = np.ascontiguousarray(block[:16])
    return bool(h[:4].view(np.uint32)[0] == MAGIC and tuple(h[4:].view(np.int32)) == (g, int(meta["k"]), int(meta["job_n"])))


def unpack(recv, metas, ncols, k_max, res_bytes, H, r, fout, fout_host=None, peer_fail=0):
    """recv: world blocks one after the other (uint8); metas: META per rank; H (rows x ld), r, fout, fout_host (or None): the
    receiver's arrays before the call; peer_fail: the word before the call, None = no word.  Returns copies after the call:
    (H, r, fout, fout_host or None, peer_fail or None)."""
    recv = np.ascontiguousarray(recv, np.uint8); metas = np.ascontiguousarray(metas, META)
    world = len(metas); bpr = recv.size // world
    assert bpr * world == recv.size and bpr >= block_bytes(res_bytes, k_max, ncols)
    H = np.array(H, np.float64, order="C"); r = np.array(r, np.float64); fout = np.array(fout, RESULT)
    fh = None if fout_host is None else np.array(fout_host, RESULT)
    Hb, rb = H.view(np.uint64), r.view(np.uint64)
    word = peer_fail
    for g in range(world):
        m = metas[g]; blk = recv[g * bpr:(g + 1) * bpr]
        k, off, lo, n = int(m["k"]), int(m["row_off"]), int(m["job_lo"]), int(m["job_n"])
        assert 0 <= k <= k_max
        if not block_is_good(blk, g, m):
            Hb[off:off + k, :ncols] = 0; rb[off:off + k] = 0
            if word is not None:
                word |= 1 << min(g, 31)
            continue
        o = HDR + res_bytes
        rows = np.ascontiguousarray(blk[o:o + 8 * k * (ncols + 1)]).view(np.uint64).reshape(k, ncols + 1)
        Hb[off:off + k, :ncols] = rows[:, :ncols]; rb[off:off + k] = rows[:, ncols]
        got = np.ascontiguousarray(blk[HDR:HDR + 32 * n]).view(RESULT)
        fout[lo:lo + n] = got
        if fh is not None:
            fh[lo:lo + n] = got
    if word is not None:
        word = int(np.array([word & 0xFFFFFFFF], np.uint32).view(np.int32)[0])      # the word is a C int: bit 31 makes it negative
    return H, r, fout, fh, word


# ---------------------------------------------------------------- inputs the tests share
def awkward_doubles(rng, shape):
    """random doubles with NaNs (two payloads), +-0, +-inf and denormals mixed in: a copy routed through arithmetic would show"""
    a = rng.normal(0, 1e3, shape)
    flat = a.reshape(-1).view(np.uint64)
    special = np.array([0x7ff8000000000000, 0x7ff4000000abcdef, 0xfff8000000000001, 0x0000000000000000, 0x8000000000000000,
                        0x0000000000000001, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000], np.uint64)
    if flat.size:
        n = max(1, flat.size // 7)
        idx = rng.choice(flat.size, size=min(n, flat.size), replace=False)
        flat[idx] = special[rng.integers(0, len(special), len(idx))]
    return a


def random_results(rng, n):
    """n RESULT records of arbitrary bytes (the kernels copy them, whatever they hold)"""
    return rng.integers(0, 256, 32 * n, dtype=np.uint8).view(RESULT).copy() if n else np.zeros(0, RESULT)


def sentinel_results(n, byte=0xA5):
    return np.full(32 * n, byte, np.uint8).view(RESULT).copy() if n else np.zeros(0, RESULT)


SENTINEL_BITS = np.uint64(0x7ff8dead0000beef)      # a NaN no kernel produces


def sentinel_doubles(shape):
    return np.full(shape, SENTINEL_BITS, np.uint64).view(np.float64)


def plan(ks, job_ns, gap_rows=0, gap_jobs=0):
    """metas for the given per-rank k and job_n, rows and jobs stacked in rank order (with optional unowned gaps in front of every
    rank's range) -> (metas, rows needed, results needed)"""
    metas = np.zeros(len(ks), META); row = job = 0
    for g, (k, n) in enumerate(zip(ks, job_ns)):
        row += gap_rows; job += gap_jobs
        metas[g] = (job, n, k, row)
        row += k; job += n
    return metas, row + gap_rows, job + gap_jobs
