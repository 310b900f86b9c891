"""The restatement of the exchange step (tests/shard_ref.py) against itself, without a GPU: unpack(concat(pack(...))) reproduces
what went in, bit for bit, and a poisoned block follows the receiver's rules.  tests/test_gpu_shard_stages.py holds k_shard_pack and
k_shard_unpack against the same functions."""
import numpy as np
import pytest

from tests import shard_ref as R


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def _case(seed, ks, job_ns, ncols, ld_pad=3, gap_rows=2, gap_jobs=1):
    rng = np.random.default_rng(seed)
    k_max = max(ks); res_bytes = R.res_bytes_for(max(job_ns)); bpr = R.block_bytes(res_bytes, k_max, ncols) + 8 * 5
    Xs = [R.awkward_doubles(rng, (k, ncols)) for k in ks]; rs = [R.awkward_doubles(rng, k) for k in ks]; res = [R.random_results(rng, n) for n in job_ns]
    blocks = [R.pack(g, Xs[g], rs[g], res[g], res_bytes, bpr, 0xEE) for g in range(len(ks))]
    metas, rows, n_fout = R.plan(ks, job_ns, gap_rows, gap_jobs)
    H0 = R.sentinel_doubles((rows, ncols + ld_pad)); r0 = R.sentinel_doubles(rows); f0 = R.sentinel_results(n_fout); fh0 = R.sentinel_results(n_fout, 0x5A)
    return dict(ks=ks, job_ns=job_ns, ncols=ncols, k_max=k_max, res_bytes=res_bytes, bpr=bpr, Xs=Xs, rs=rs, res=res, blocks=blocks, metas=metas,
                H0=H0, r0=r0, f0=f0, fh0=fh0)


def test_pack_lays_the_block_out_as_documented():
    c = _case(1, [3], [5], 4)
    b = c["blocks"][0]
    assert b.size == c["bpr"] and c["res_bytes"] == 256
    assert b[:4].view(np.uint32)[0] == 0x4c564b58 and tuple(b[4:16].view(np.int32)) == (0, 3, 5)
    assert np.all(b[16:256] == 0xEE)                                              # header bytes beyond the 16 defined ones
    assert np.array_equal(b[256:256 + 160], _bits(c["res"][0])) and np.all(b[256 + 160:512] == 0xEE)
    rows = b[512:512 + 3 * 5 * 8].view(np.uint64).reshape(3, 5)
    assert np.array_equal(rows[:, :4], c["Xs"][0].view(np.uint64)) and np.array_equal(rows[:, 4], c["rs"][0].view(np.uint64))
    assert np.all(b[512 + 120:] == 0xEE)


@pytest.mark.parametrize("ks,job_ns,ncols", [([3], [5], 4), ([0, 7, 2], [0, 300, 1], 1), ([0, 0], [0, 0], 9), ([2] * 33, [1] * 33, 257)])
def test_unpack_of_packed_blocks_reproduces_the_inputs(ks, job_ns, ncols):
    c = _case(2, ks, job_ns, ncols)
    for with_host in (True, False):
        H, r, f, fh, word = R.unpack(np.concatenate(c["blocks"]), c["metas"], ncols, c["k_max"], c["res_bytes"], c["H0"], c["r0"], c["f0"],
                                     c["fh0"] if with_host else None, 0)
        assert word == 0 and (fh is None) == (not with_host)
        owned_rows = np.zeros(len(r), bool); owned_jobs = np.zeros(len(f), bool)
        for g, m in enumerate(c["metas"]):
            sl = slice(int(m["row_off"]), int(m["row_off"]) + ks[g]); js = slice(int(m["job_lo"]), int(m["job_lo"]) + job_ns[g])
            assert np.array_equal(H[sl, :ncols].view(np.uint64), c["Xs"][g].view(np.uint64)) and np.array_equal(r[sl].view(np.uint64), c["rs"][g].view(np.uint64))
            assert np.array_equal(_bits(f[js]), _bits(c["res"][g])) and (fh is None or np.array_equal(_bits(fh[js]), _bits(c["res"][g])))
            owned_rows[sl] = True; owned_jobs[js] = True
        # the sentinel survives wherever no rank owns: padding columns, gap rows, gap results
        assert np.all(H.view(np.uint64)[:, ncols:] == R.SENTINEL_BITS) and np.all(H.view(np.uint64)[~owned_rows] == R.SENTINEL_BITS)
        assert np.all(r.view(np.uint64)[~owned_rows] == R.SENTINEL_BITS)
        assert np.array_equal(_bits(f[~owned_jobs]), _bits(c["f0"][~owned_jobs]))
        assert fh is None or np.array_equal(_bits(fh[~owned_jobs]), _bits(c["fh0"][~owned_jobs]))
        assert np.all(c["H0"].view(np.uint64) == R.SENTINEL_BITS)                  # the inputs are not modified


def _poison(block, field):
    b = block.copy(); w = b[:16].view(np.int32)
    if field == "ff":
        b[:256] = 0xFF
    else:
        w[{"magic": 0, "rank": 1, "k": 2, "n_res": 3}[field]] += 1
    return b


@pytest.mark.parametrize("field", ["magic", "rank", "k", "n_res", "ff"])
def test_a_poisoned_block_zeroes_its_rows_keeps_its_results_out_and_raises_its_bit(field):
    ks, job_ns, ncols = [2, 3, 1], [4, 2, 3], 5
    c = _case(3, ks, job_ns, ncols)
    good = R.unpack(np.concatenate(c["blocks"]), c["metas"], ncols, c["k_max"], c["res_bytes"], c["H0"], c["r0"], c["f0"], c["fh0"], 0)
    bad = 1
    blocks = list(c["blocks"]); blocks[bad] = _poison(blocks[bad], field)
    assert not R.block_is_good(blocks[bad], bad, c["metas"][bad]) and R.block_is_good(c["blocks"][bad], bad, c["metas"][bad])
    H, r, f, fh, word = R.unpack(np.concatenate(blocks), c["metas"], ncols, c["k_max"], c["res_bytes"], c["H0"], c["r0"], c["f0"], c["fh0"], 0)
    m = c["metas"][bad]; sl = slice(int(m["row_off"]), int(m["row_off"]) + ks[bad]); js = slice(int(m["job_lo"]), int(m["job_lo"]) + job_ns[bad])
    assert word == 1 << bad
    assert np.all(H.view(np.uint64)[sl, :ncols] == 0) and np.all(r.view(np.uint64)[sl] == 0)
    assert np.all(H.view(np.uint64)[sl, ncols:] == R.SENTINEL_BITS)
    assert np.array_equal(_bits(f[js]), _bits(c["f0"][js])) and np.array_equal(_bits(fh[js]), _bits(c["fh0"][js]))
    # every other rank, and everything unowned, is as in the healthy run
    keep_r = np.ones(len(r), bool); keep_r[sl] = False; keep_j = np.ones(len(f), bool); keep_j[js] = False
    assert np.array_equal(H.view(np.uint64)[keep_r], good[0].view(np.uint64)[keep_r]) and np.array_equal(r.view(np.uint64)[keep_r], good[1].view(np.uint64)[keep_r])
    assert np.array_equal(_bits(f[keep_j]), _bits(good[2][keep_j])) and np.array_equal(_bits(fh[keep_j]), _bits(good[3][keep_j]))


def test_peer_word_two_bad_ranks_the_clamp_at_31_and_no_word():
    ks = [1] * 33; job_ns = [1] * 33; ncols = 2
    c = _case(4, ks, job_ns, ncols)
    blocks = list(c["blocks"])
    for g in (3, 7):
        blocks[g] = _poison(blocks[g], "k")
    word = R.unpack(np.concatenate(blocks), c["metas"], ncols, 1, c["res_bytes"], c["H0"], c["r0"], c["f0"], None, 0)[4]
    assert word == (1 << 3) | (1 << 7)
    for bad in ([31], [32], [31, 32]):
        blocks = list(c["blocks"])
        for g in bad:
            blocks[g] = _poison(blocks[g], "magic")
        word = R.unpack(np.concatenate(blocks), c["metas"], ncols, 1, c["res_bytes"], c["H0"], c["r0"], c["f0"], None, 0)[4]
        assert word == -2 ** 31                                                    # bit 31 of a C int
    H, r, f, fh, word = R.unpack(np.concatenate(blocks), c["metas"], ncols, 1, c["res_bytes"], c["H0"], c["r0"], c["f0"], None, None)
    assert word is None and all(np.all(H.view(np.uint64)[int(c["metas"][g]["row_off"]), :ncols] == 0) for g in (31, 32))
    # a word that already holds bits keeps them
    assert R.unpack(np.concatenate(c["blocks"]), c["metas"], ncols, 1, c["res_bytes"], c["H0"], c["r0"], c["f0"], None, 0x10)[4] == 0x10
