"""k_shard_pack and k_shard_unpack (larvio_amd/csrc/be_shard.hip), the kernels around the all-gather of the sharded update, launched
through the stage entries lvk_shard_pack_stage / lvk_shard_unpack_stage and held against the numpy restatement tests/shard_ref.py.
The kernels only copy, so every comparison is exact, on bit patterns; the inputs carry NaNs with payloads, +-0, infinities and
denormals (a copy routed through arithmetic would show), the receiver's arrays a sentinel (a write outside the layout would show).
Shapes: ncols around the 256-column trip of the row loops, k and job counts of 0, results across the 4096-record threshold of the
pack kernel's grid-stride copy, worlds beyond the 31 bits of the peer-failure word."""
import ctypes as C

import numpy as np
import pytest

from tests import shard_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG = 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("ld_pad", [0, 5])
@pytest.mark.parametrize("ncols", [1, 255, 256, 257, 600])
def test_pack_writes_the_documented_block_and_nothing_else(gpu_ctx, ncols, ld_pad):
    """every k x n_res x rank at this row shape; the block is compared byte for byte with the restatement, whose undefined bytes
    (header 16..255, the padding of the result area, rows k..k_max-1, the tail) hold the fill byte"""
    from larvio_amd import larvio as lv
    rng = np.random.default_rng(100 * ncols + ld_pad)
    ld = ncols + ld_pad
    Xbuf = R.awkward_doubles(rng, (65, ld)); rX = R.awkward_doubles(rng, 65); res_all = R.random_results(rng, 20000)
    n_calls = 0
    for k in (0, 1, 7, 65):
        for n_res in (0, 1, 63, 64, 65, 4096, 4097, 20000):
            res_bytes = R.res_bytes_for(n_res + 3)                                 # room for padding after the last result
            bpr = R.block_bytes(res_bytes, k + 2, ncols) + 64                      # k_max = k + 2, and a tail
            for rank in (0, 5, 40):
                fill = (0xC3, 0x00, 0xFF)[n_calls % 3]
                got = lv.shard_pack(gpu_ctx, rank, Xbuf[:k], rX[:k], res_all[:n_res], res_bytes, bpr, fill, ncols=ncols)
                want = R.pack(rank, Xbuf[:k, :ncols], rX[:k], res_all[:n_res], res_bytes, bpr, fill)
                if not np.array_equal(got, want):
                    bad = np.flatnonzero(got != want)
                    o_rows = R.HDR + res_bytes
                    pytest.fail("k %d n_res %d rank %d: %d bytes differ, first at %d (header < 256 <= results < %d <= rows < %d <= undefined)"
                                % (k, n_res, rank, bad.size, bad[0], o_rows, o_rows + 8 * k * (ncols + 1)))
                n_calls += 1
    assert n_calls == 96


# ------------------------------------------------------------------------------------------------------------------------- unpack
_KS = {1: [5], 2: [0, 5], 3: [3, 0, 5], 8: [2, 5, 0, 1, 5, 4, 0, 3]}
_JOBS = {1: [300], 2: [0, 300], 3: [7, 300, 0], 8: [1, 0, 257, 300, 2, 0, 64, 256]}
_CASES = {}


def _healthy_case(world, ncols):
    """the blocks of `world` ranks, the receiver's plan and sentinel-filled arrays, and the restatement's answer - built once"""
    key = (world, ncols)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * world + ncols)
    if world in _KS:
        ks, job_ns = _KS[world], _JOBS[world]
    else:                                                                          # 33 ranks: 0, k_max and everything between, job counts likewise
        ks = [(0, 5, 2, 4, 1, 3)[g % 6] for g in range(world)]; job_ns = [(3, 0, 300, 1, 257, 0, 12)[g % 7] for g in range(world)]
    k_max = max(ks); res_bytes = R.res_bytes_for(max(job_ns)); bpr = R.block_bytes(res_bytes, k_max, ncols)
    Xs = [R.awkward_doubles(rng, (k, ncols)) for k in ks]; rs = [R.awkward_doubles(rng, k) for k in ks]; res = [R.random_results(rng, n) for n in job_ns]
    # what a sender leaves undefined (rows k.., padding) arrives as arbitrary bytes
    blocks = [R.pack(g, Xs[g], rs[g], res[g], res_bytes, bpr, 0x3C + g) for g in range(world)]
    metas, rows, n_fout = R.plan(ks, job_ns, gap_rows=1, gap_jobs=2)
    c = dict(world=world, ncols=ncols, ks=ks, job_ns=job_ns, k_max=k_max, res_bytes=res_bytes, bpr=bpr, blocks=blocks, metas=metas,
             H0=R.sentinel_doubles((rows, ncols + 3)), r0=R.sentinel_doubles(rows), f0=R.sentinel_results(n_fout), fh0=R.sentinel_results(n_fout, 0x5A))
    c["want"] = R.unpack(np.concatenate(blocks), metas, ncols, k_max, res_bytes, c["H0"], c["r0"], c["f0"], c["fh0"], 0)
    for a in (c["H0"], c["r0"], c["f0"], c["fh0"], metas, *blocks, *c["want"][:4]):
        a.setflags(write=False)
    _CASES[key] = c
    return c


def _run_unpack(ctx, c, blocks=None, with_host=True, peer_fail=0):
    from larvio_amd import larvio as lv
    return lv.shard_unpack(ctx, np.concatenate(c["blocks"] if blocks is None else blocks), c["metas"], c["ncols"], c["k_max"], c["res_bytes"], c["H0"], c["r0"],
                           c["f0"], c["fh0"] if with_host else None, peer_fail)


def _assert_same(got, want, what):
    H, r, f, fh, word = got
    assert np.array_equal(_u64(H), _u64(want[0])), what + ": H"
    assert np.array_equal(_u64(r), _u64(want[1])), what + ": r"
    assert np.array_equal(_bits(f), _bits(want[2])), what + ": results"
    assert (fh is None) == (want[3] is None) and (fh is None or np.array_equal(_bits(fh), _bits(want[3]))), what + ": host mirror of the results"
    assert word == want[4], what + ": peer-failure word %r, expected %r" % (word, want[4])


@pytest.mark.parametrize("with_host", [True, False])
@pytest.mark.parametrize("ncols", [1, 257])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 33])
def test_unpack_of_healthy_blocks_equals_the_restatement(gpu_ctx, world, ncols, with_host):
    """per-rank k from 0 to k_max, job counts from 0 to beyond 256, ld > ncols, unowned rows and results between the ranks' ranges:
    rows, residuals and results land where the plan says, the sentinel survives everywhere else, no peer bit"""
    c = _healthy_case(world, ncols)
    assert 0 in c["ks"] or world == 1
    assert c["k_max"] in c["ks"] and max(c["job_ns"]) > 256 and (0 in c["job_ns"] or world == 1)
    want = c["want"] if with_host else c["want"][:3] + (None, 0)
    _assert_same(_run_unpack(gpu_ctx, c, with_host=with_host), want, "world %d" % world)
    # the restatement left the sentinel wherever no rank owns, so the comparison above covers it; say so once, explicitly
    assert np.all(_u64(want[0])[:, ncols:] == R.SENTINEL_BITS) and np.all(_u64(want[0])[0] == R.SENTINEL_BITS) and want[4] == 0


@pytest.mark.parametrize("world", [1, 2, 3, 8, 33])
def test_unpack_with_no_rows_anywhere(gpu_ctx, world):
    """k == 0 on every rank, k_max == 0: a grid of one block per rank, which only copies results"""
    from larvio_amd import larvio as lv
    rng = np.random.default_rng(world)
    ncols = 257; job_ns = [(2, 0, 300)[g % 3] for g in range(world)]; ks = [0] * world
    res_bytes = R.res_bytes_for(max(job_ns)); bpr = R.block_bytes(res_bytes, 0, ncols)
    res = [R.random_results(rng, n) for n in job_ns]
    blocks = [R.pack(g, np.zeros((0, ncols)), np.zeros(0), res[g], res_bytes, bpr, 0x11) for g in range(world)]
    metas, rows, n_fout = R.plan(ks, job_ns, gap_rows=1, gap_jobs=1)
    H0 = R.sentinel_doubles((rows, ncols + 1)); r0 = R.sentinel_doubles(rows); f0 = R.sentinel_results(n_fout); fh0 = R.sentinel_results(n_fout, 0x5A)
    want = R.unpack(np.concatenate(blocks), metas, ncols, 0, res_bytes, H0, r0, f0, fh0, 0)
    got = lv.shard_unpack(gpu_ctx, np.concatenate(blocks), metas, ncols, 0, res_bytes, H0, r0, f0, fh0, 0)
    _assert_same(got, want, "world %d, k_max 0" % world)
    assert np.all(_u64(got[0]) == R.SENTINEL_BITS) and np.all(_u64(got[1]) == R.SENTINEL_BITS)


def _poison(block, field):
    """the block with exactly one header field altered - or, "ff", its whole header overwritten as a rank that failed locally does"""
    b = block.copy()
    if field == "ff":
        b[:R.HDR] = 0xFF
    else:
        b[:16].view(np.int32)[{"magic": 0, "rank": 1, "k": 2, "n_res": 3}[field]] += 1
    return b


def _assert_poisoned(c, got, bad, what, word):
    """rank(s) `bad`: rows and residuals zero, results untouched; everything else as in the healthy run; the word as given"""
    H, r, f, fh, w = got
    ncols = c["ncols"]; keep_r = np.ones(len(r), bool); keep_j = np.ones(len(f), bool)
    for g in bad:
        m = c["metas"][g]; sl = slice(int(m["row_off"]), int(m["row_off"]) + c["ks"][g]); js = slice(int(m["job_lo"]), int(m["job_lo"]) + c["job_ns"][g])
        assert np.all(_u64(H)[sl, :ncols] == 0) and np.all(_u64(r)[sl] == 0), what + ": rows of rank %d not zero" % g
        assert np.all(_u64(H)[sl, ncols:] == R.SENTINEL_BITS), what + ": padding columns of rank %d's rows" % g
        assert np.array_equal(_bits(f[js]), _bits(c["f0"][js])), what + ": results of rank %d were copied" % g
        assert fh is None or np.array_equal(_bits(fh[js]), _bits(c["fh0"][js])), what + ": results of rank %d were copied to the host mirror" % g
        keep_r[sl] = False; keep_j[js] = False
    want = c["want"]
    assert np.array_equal(_u64(H)[keep_r], _u64(want[0])[keep_r]) and np.array_equal(_u64(r)[keep_r], _u64(want[1])[keep_r]), what + ": another rank's rows"
    assert np.array_equal(_bits(f[keep_j]), _bits(want[2][keep_j])), what + ": another rank's results"
    assert fh is None or np.array_equal(_bits(fh[keep_j]), _bits(want[3][keep_j])), what + ": another rank's results (host mirror)"
    assert w == word, what + ": peer-failure word %r, expected %r" % (w, word)


def _bit(g):
    return int(np.array([1 << min(g, 31)], np.uint32).view(np.int32)[0])


@pytest.mark.parametrize("field", ["magic", "rank", "k", "n_res", "ff"])
@pytest.mark.parametrize("world", [2, 3, 33])
def test_unpack_rejects_a_block_whose_header_differs_in_one_field(gpu_ctx, world, field):
    """one rank at a time, one field at a time (and the 0xFF header of a rank that failed locally): that rank's rows and residuals
    are zero, its results still hold the sentinel, every other rank is as in the healthy run, the word holds exactly its bit -
    bit 31 for ranks 31 and 32 alike"""
    c = _healthy_case(world, 257)
    for g in range(world):
        blocks = list(c["blocks"]); blocks[g] = _poison(blocks[g], field)
        got = _run_unpack(gpu_ctx, c, blocks)
        _assert_poisoned(c, got, [g], "world %d, rank %d, %s" % (world, g, field), _bit(g))
        # the restatement agrees with the rules spelled out above
        _assert_same(got, R.unpack(np.concatenate(blocks), c["metas"], 257, c["k_max"], c["res_bytes"], c["H0"], c["r0"], c["f0"], c["fh0"], 0), "restatement")


def test_unpack_two_bad_ranks_give_two_bits_and_ranks_31_and_32_share_bit_31(gpu_ctx):
    c = _healthy_case(33, 257)
    for bad, word in (([1, 4], 0x12), ([0, 30], 1 | (1 << 30)), ([31, 32], _bit(31)), ([32], _bit(31)), ([5, 32], (1 << 5) | _bit(31))):
        blocks = list(c["blocks"])
        for g, field in zip(bad, ("k", "ff")):
            blocks[g] = _poison(blocks[g], field)
        _assert_poisoned(c, _run_unpack(gpu_ctx, c, blocks), bad, "bad ranks %s" % bad, word)
    c3 = _healthy_case(3, 257)
    blocks = [_poison(b, "magic") for b in c3["blocks"]]
    _assert_poisoned(c3, _run_unpack(gpu_ctx, c3, blocks), [0, 1, 2], "all three bad", 7)
    # bits already in the word stay
    blocks = list(c3["blocks"]); blocks[2] = _poison(blocks[2], "n_res")
    _assert_poisoned(c3, _run_unpack(gpu_ctx, c3, blocks, peer_fail=0x100), [2], "word pre-set", 0x104)


@pytest.mark.parametrize("world", [2, 33])
def test_unpack_without_a_peer_failure_word_still_zeroes_the_rows(gpu_ctx, world):
    from larvio_amd import larvio as lv
    c = _healthy_case(world, 257)
    g = world - 1 if c["ks"][world - 1] else int(np.argmax(c["ks"]))
    assert c["ks"][g] > 0
    blocks = list(c["blocks"]); blocks[g] = _poison(blocks[g], "ff")
    got = lv.shard_unpack(gpu_ctx, np.concatenate(blocks), c["metas"], 257, c["k_max"], c["res_bytes"], c["H0"], c["r0"], c["f0"], c["fh0"], None)
    _assert_poisoned(c, got, [g], "no word, rank %d" % g, None)


# ------------------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_errors_launch_nothing_and_leave_the_context_usable(gpu_ctx):
    from larvio_amd import larvio as lv
    from larvio_amd._lib import LvkError
    L = lv._L()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ncols, k, n_res = 4, 3, 5
    X = np.ones((k, ncols + 2)); rX = np.ones(k); res = R.sentinel_results(n_res); out = np.full(4096, 0x77, np.uint8)
    ok_rb, ok_bpr = 256, R.block_bytes(256, k, ncols)

    def pack(rank=0, ld=ncols + 2, k=k, ncols=ncols, n_res=n_res, res_bytes=ok_rb, bpr=ok_bpr):
        return L.lvk_shard_pack_stage(gpu_ctx.h, rank, vp(X), ld, vp(rX), k, ncols, vp(res), n_res, res_bytes, 0, vp(out), bpr)

    assert pack() == 0
    out[:] = 0x77
    for kw in (dict(k=-1), dict(ncols=-1), dict(n_res=-1), dict(rank=-1), dict(ld=ncols - 1), dict(res_bytes=255), dict(res_bytes=128), dict(res_bytes=0),
               dict(n_res=9, res_bytes=256), dict(bpr=ok_bpr - 8), dict(bpr=R.HDR), dict(bpr=0), dict(bpr=ok_bpr + 4)):
        assert pack(**kw) == ERR_ARG, kw
    assert np.all(out == 0x77)                                                     # nothing came back: nothing ran

    ks, job_ns = [2, 1], [3, 2]
    metas, rows, n_fout = R.plan(ks, job_ns)
    res_bytes = 256; bpr = R.block_bytes(res_bytes, 2, ncols)
    rng = np.random.default_rng(0)
    blocks = [R.pack(g, R.awkward_doubles(rng, (ks[g], ncols)), R.awkward_doubles(rng, ks[g]), R.random_results(rng, job_ns[g]), res_bytes, bpr, 0) for g in range(2)]
    recv = np.concatenate(blocks)
    H0 = R.sentinel_doubles((rows, ncols + 1)); r0 = R.sentinel_doubles(rows); f0 = R.sentinel_results(n_fout); fh0 = R.sentinel_results(n_fout, 0x5A)
    H = H0.copy(); r = r0.copy(); f = f0.copy(); fh = fh0.copy(); word = np.zeros(1, np.int32)

    def unpack(metas=metas, world=2, ncols=ncols, k_max=2, res_bytes=res_bytes, bpr=bpr, ld=ncols + 1, rows=rows, n_fout=n_fout):
        m = np.ascontiguousarray(metas, R.META)
        return L.lvk_shard_unpack_stage(gpu_ctx.h, vp(recv), bpr, vp(m), world, ncols, k_max, res_bytes, vp(H), ld, rows, vp(r), vp(f), vp(fh), n_fout, vp(word))

    def meta(g, **kw):
        m = metas.copy()
        for key, v in kw.items():
            m[g][key] = v
        return m

    bad = [dict(world=0), dict(world=-1), dict(ncols=-1), dict(k_max=-1), dict(rows=-1), dict(n_fout=-1), dict(ld=ncols - 1), dict(res_bytes=255), dict(res_bytes=128),
           dict(bpr=bpr - 8), dict(bpr=bpr + 4), dict(bpr=0),
           dict(k_max=1),                                                          # rank 0's k = 2 exceeds k_max
           dict(rows=rows - 1), dict(n_fout=n_fout - 1),                           # the last rank's rows / jobs leave the arrays
           dict(metas=meta(0, k=-1)), dict(metas=meta(0, k=3)), dict(metas=meta(1, row_off=-1)), dict(metas=meta(1, row_off=rows)),
           dict(metas=meta(1, job_lo=-1)), dict(metas=meta(1, job_n=-1)), dict(metas=meta(1, job_lo=n_fout - 1)), dict(metas=meta(0, job_n=9, job_lo=0), n_fout=64)]
    for kw in bad:
        assert unpack(**kw) == ERR_ARG, kw
    assert np.all(_u64(H) == R.SENTINEL_BITS) and np.all(_u64(r) == R.SENTINEL_BITS) and np.array_equal(_bits(f), _bits(f0)) and word[0] == 0
    with pytest.raises(LvkError, match="lvk status 1"):
        lv.shard_unpack(gpu_ctx, recv, metas, ncols, 1, res_bytes, H0, r0, f0, fh0, 0)
    # the context is intact: the same call with good arguments, and a healthy case of the suite
    assert unpack() == 0
    _assert_same((H, r, f, fh, int(word[0])), R.unpack(recv, metas, ncols, 2, res_bytes, H0, r0, f0, fh0, 0), "after the refused calls")
    c = _healthy_case(3, 257)
    _assert_same(_run_unpack(gpu_ctx, c), c["want"], "healthy case after the refused calls")
