"""The sharded measurement update as a product path (lvk_ekf_set_shard; SURVEY 8e, BASELINE.json configs[4]) on ONE GPU: two
processes = two ranks share device 0, each runs the whole filter on the same simulated feature messages and does the per-feature
device work of its own contiguous slice; the all-gather of the compressed blocks goes through the host over gloo (RCCL refuses two
ranks on one device - on a multi-GPU node bench.py --sharded uses lvk_shard_allgather_rccl instead, same pack / unpack kernels).
Required: both ranks end with IDENTICAL bits (state, covariance, clone and feature ids, gate counters), equal to the unsharded
filter within the parity tolerance, and the exchange really happened.

Below those: the same product path in ONE process.  Worlds 3 and 4 run in lock step, one thread and one context per rank, the
all-gather a barrier through host memory; and the failure paths lvk_ekf_set_shard promises - a peer whose block arrives poisoned
and a transport that fails end the update with an error instead of a wait - are driven by an exchange callback that plays the
missing peer.  Every wait in them carries a timeout."""
import ctypes as C
import os
import threading
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _sim():
    from tests import feature_sim as F
    return F.simulate(11, t0=2.0, t1=6.0, max_feat=900, n_per_batch=260, sw_size=24, max_features_in_one_grid=1, estimate_td=1, estimate_extrin=1,
                      max_features=900)


def _run(be, sim):
    from tests import feature_sim as F
    out = []
    n = F.drive(_Wrap(be), sim, on_update=lambda ts: None)
    s = be.state()
    return n, s, be.cov(), be.clones()["id"].copy(), be.features()[0].copy(), be.counters()


class _Wrap:
    """the oracle's (process, set_state) spelling on top of larvio_amd.LarVio"""

    def __init__(self, be):
        self.be = be

    def set_state(self, *a):
        self.be.set_state(*a)

    def process(self, ts, m, imu):
        upd, rest = self.be.processFeatures((ts, m), imu)
        return upd, len(imu) - len(rest)


def _worker(rank, world, port, q):
    try:
        import torch.distributed as dist
        import larvio_amd
        from larvio_amd import sharding
        os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sim = _sim()
        ctx = larvio_amd.Context(0)
        be = larvio_amd.LarVio(sim["cfg"], ctx); assert be.initialize()
        ex = sharding.HostExchange(ctx, dist, rank, world)
        be.set_shard(*ex.args())
        n, s, P, cid, fid, cnt = _run(be, sim)
        st = be.shard_stats()
        q.put((rank, n, {k: np.array(v) for k, v in s.items()}, P, cid, fid, cnt, st, ex.calls))
        dist.barrier()
        be.close(); ctx.close()
        dist.destroy_process_group()
    except Exception as exc:                                  # surface the failure instead of a queue timeout
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise


def test_two_ranks_on_one_gpu_are_bit_identical_and_match_the_unsharded_filter(gpu_ctx):
    import torch.multiprocessing as mp
    import larvio_amd
    sim = _sim()
    ref = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert ref.initialize()
    n_ref, s_ref, P_ref, cid_ref, fid_ref, cnt_ref = _run(ref, sim)
    ref.close()
    assert n_ref >= 38 and cnt_ref["hybrid"] >= 30
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 1500)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    for _ in range(2):
        item = q.get(timeout=600)
        assert item[1] != "error", item[2]
        res.append(item)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    res.sort(key=lambda t: t[0])
    a, b = res
    assert a[1] == b[1] == n_ref
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k]), k                                # replicas: identical bits
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]) and a[6] == b[6]
    rel = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300))
    worst = max(rel(a[2][k], s_ref[k]) for k in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"))
    assert worst < 1e-6 and rel(a[3], P_ref) < 1e-6, (worst, rel(a[3], P_ref))   # vs the unsharded filter: another reduction tree, same information
    assert np.array_equal(a[4], cid_ref) and np.array_equal(a[5], fid_ref)
    for k in ("hybrid", "msckf", "gated_in", "gated_out", "map"):
        assert a[6][k] == cnt_ref[k], (k, a[6], cnt_ref)
    for r in (a, b):
        st = r[7]
        # ONE all-gather per sharded update, also when new features enter the state (their gate is computed on every rank)
        assert st["sharded_updates"] >= 30 and st["exchanges"] == st["sharded_updates"] and st["exchanges"] == r[8] and st["bytes_sent"] > 0
    assert 0.25 < a[7]["rows_stacked"] / max(a[7]["rows_stacked"] + b[7]["rows_stacked"], 1) < 0.75   # the rows really were split
    print("sharded x2 on one GPU: updates", n_ref, "worst rel vs unsharded", worst, rel(a[3], P_ref), a[7], b[7])


def test_rccl_transport_executes_at_world_one(gpu_ctx):
    """The built-in transport on hardware: lvk_shard_unique_id -> lvk_shard_comm_create(rank 0, world 1) (ncclCommInitRank through the
    late-bound librccl) -> lvk_shard_allgather_rccl on device buffers, enqueued on the context's own stream; the bytes must arrive."""
    import ctypes as C
    from larvio_amd import sharding
    from larvio_amd._lib import lib
    uid = sharding.unique_id()
    assert len(uid) == 128 and any(uid)
    sh = sharding.RcclShard(gpu_ctx, 0, 1, uid)
    L = lib()
    L.lvk_shard_allgather_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]; L.lvk_shard_allgather_rccl.restype = C.c_int
    L.lvk_shard_comm_error.argtypes = [C.c_void_p]; L.lvk_shard_comm_error.restype = C.c_char_p
    rng = np.random.default_rng(3)
    for n in (256, 600_000):
        src = rng.integers(0, 256, n).astype(np.uint8)
        d_s = gpu_ctx.to_device(src); d_r = gpu_ctx.to_device(np.zeros(n, np.uint8))
        rc = L.lvk_shard_allgather_rccl(sh._h, C.c_void_p(d_s.ptr), C.c_void_p(d_r.ptr), n, C.c_void_p(gpu_ctx.stream))
        assert rc == 0, L.lvk_shard_comm_error(sh._h)
        gpu_ctx.sync()
        assert np.array_equal(gpu_ctx.to_host(d_r, np.uint8, (n,)), src)
    sh.close()


def test_sharded_filter_through_rccl_at_world_one_equals_the_unsharded_filter(gpu_ctx):
    """lvk_ekf_set_shard(rank 0, world 1, lvk_shard_allgather_rccl): the filter takes the sharded branch - per-rank rows, first
    compression stage, k_shard_pack -> ncclAllGather -> k_shard_unpack, replicated second stage - with RCCL as the transport on one
    GPU, through 40 updates including the ones that admit new in-state features, and must agree with the unsharded filter
    (another reduction tree, same information) with identical discrete decisions; one exchange per sharded update."""
    import larvio_amd
    from larvio_amd import sharding
    sim = _sim()
    ref = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert ref.initialize()
    n_ref, s_ref, P_ref, cid_ref, fid_ref, cnt_ref = _run(ref, sim)
    ref.close()
    be = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert be.initialize()
    sh = sharding.RcclShard(gpu_ctx, 0, 1, sharding.unique_id())
    be.set_shard(*sh.args())
    n, s, P, cid, fid, cnt = _run(be, sim)
    st = be.shard_stats()
    be.close(); sh.close()
    rel = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300))
    worst = max(rel(s[k], s_ref[k]) for k in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"))
    assert n == n_ref and worst < 1e-7 and rel(P, P_ref) < 1e-7, (n, n_ref, worst, rel(P, P_ref))
    assert np.array_equal(cid, cid_ref) and np.array_equal(fid, fid_ref)
    for k in ("hybrid", "msckf", "gated_in", "gated_out", "map"):
        assert cnt[k] == cnt_ref[k], (k, cnt, cnt_ref)
    assert st["sharded_updates"] >= 30 and st["exchanges"] == st["sharded_updates"] and st["bytes_sent"] > 0 and st["rows_stacked"] > 0, st
    print("sharded through RCCL at world 1: updates", n, "worst rel vs unsharded", worst, rel(P, P_ref), st)


# ------------------------------------------------------------------------------------------ one process: failure paths, worlds 3 and 4
# The smallest run that shards: 150 tracked features of a 120-per-batch landmark cloud, a 12-clone window, 1.5 s = 15 feature messages.
# Tracks are lost from the second message on, so the filter runs a sharded update within its first few messages (asserted below), and
# the window fills after 12, which adds the pruning updates.
_SMALL = dict(seed=11, t0=2.0, t1=3.5, max_feat=150, n_per_batch=120, sw_size=12)
_WAIT = 60.0                                              # seconds, against an exchange of milliseconds
_small_cache = {}


def _small_sim():
    from tests import feature_sim as F
    if "sim" not in _small_cache:
        kw = dict(_SMALL); seed = kw.pop("seed")
        _small_cache["sim"] = F.simulate(seed, **kw)
    return _small_cache["sim"]


def _small_ref(gpu_ctx):
    """the unsharded filter on the small run: (updates, state, P, clone ids, feature ids, counters), computed once"""
    import larvio_amd
    if "ref" not in _small_cache:
        sim = _small_sim()
        ref = larvio_amd.LarVio(sim["cfg"], gpu_ctx); assert ref.initialize()
        _small_cache["ref"] = _run(ref, sim)
        ref.close()
    return _small_cache["ref"]


def _header_k(block):
    """k of a block on the wire (include/lvk_c.h: magic, rank, k, n_res)"""
    return int(np.ascontiguousarray(block[:16]).view(np.int32)[2])


class _LonelyRank:
    """Exchange callback of rank 0 of world 2 when there is no rank 1: it moves its own block into slot 0 of d_recv through the host,
    as sharding.HostExchange does, and writes slot 1 itself - `peer` decides with what.  fail_first: return an error on the first
    call instead, as a transport that broke."""

    def __init__(self, ctx, peer=None, fail_first=False):
        from larvio_amd import sharding
        self.ctx, self.peer, self.fail_first = ctx, peer, fail_first
        self.calls = 0; self.aborts = 0; self.sizes = []
        self._cb = sharding.EXCHANGE_FN(self._call)

    def _call(self, user, d_send, d_recv, nbytes, stream):
        from larvio_amd._lib import lib
        try:
            self.calls += 1
            if nbytes == 0:
                self.aborts += 1
                return 2
            if self.fail_first and self.calls == 1:
                return 2
            L = lib()
            self.ctx.sync()
            mine = np.empty(nbytes, np.uint8)
            self.ctx.check(L.lvk_memcpy_d2h(self.ctx.h, mine.ctypes.data_as(C.c_void_p), C.c_void_p(d_send), nbytes))
            allb = np.concatenate([mine, self.peer(mine)])
            assert allb.size == 2 * nbytes
            self.ctx.check(L.lvk_memcpy_h2d(self.ctx.h, C.c_void_p(d_recv), allb.ctypes.data_as(C.c_void_p), allb.nbytes))
            self.ctx.sync()
            self.sizes.append(nbytes)
            return 0
        except Exception as exc:                                  # never let an exception cross the C frame
            print("_LonelyRank failed:", repr(exc))
            return 2

    def args(self):
        return 0, 2, C.cast(self._cb, C.c_void_p), None, self


def _drive_until_error(be, sim, ex):
    """feed messages until processFeatures raises; a call during which the exchange ran must be the one that raises
    -> (the error or None, messages fed before it)"""
    from larvio_amd import LvkError
    imu = sim["imu"]; lo = 0
    be.set_state(*sim["init"])
    for i, (ts, m) in enumerate(sim["msgs"]):
        hi = int(np.searchsorted(imu["t"], ts + 0.05, side="left"))
        before = ex.calls
        try:
            _, rest = be.processFeatures((ts, m), imu[lo:hi])
        except LvkError as err:
            assert ex.calls == before + 1, "processFeatures raised without having reached the exchange: %s" % err
            return err, i
        assert ex.calls == before, "message %d: the update went through the exchange and returned without an error" % i
        lo += (hi - lo) - len(rest)
    return None, len(sim["msgs"])


def _assert_context_still_runs_the_unsharded_filter(ctx, gpu_ctx):
    import larvio_amd
    sim = _small_sim()
    n_ref, s_ref, P_ref, cid_ref, fid_ref, cnt_ref = _small_ref(gpu_ctx)
    be = larvio_amd.LarVio(sim["cfg"], ctx); assert be.initialize()
    n, s, P, cid, fid, cnt = _run(be, sim)
    be.close()
    assert n == n_ref and cnt == cnt_ref and np.array_equal(cid, cid_ref) and np.array_equal(fid, fid_ref), (n, n_ref, cnt, cnt_ref)      # unsharded both: every counter


@pytest.mark.parametrize("how", ["poisoned_peer", "failing_transport"])
def test_a_failed_peer_or_transport_ends_the_update_with_an_error(gpu_ctx, how):
    """poisoned_peer: rank 1's block arrives as 0xFF bytes (what a rank that failed locally posts over its header) - the
    processFeatures call of that very update raises LVK_ERR_DEVICE naming peer mask 0x2.  failing_transport: the callback returns an
    error on its first call - that call raises "the exchange callback failed".  Either way the call returns (rank 0 has nobody to wait
    for), and a fresh filter on the same context then runs the unsharded simulation to the reference's counters."""
    import larvio_amd
    sim = _small_sim()
    ctx = larvio_amd.Context(0)
    try:
        be = larvio_amd.LarVio(sim["cfg"], ctx); assert be.initialize()
        ex = _LonelyRank(ctx, peer=lambda mine: np.full(mine.size, 0xFF, np.uint8), fail_first=(how == "failing_transport"))
        be.set_shard(*ex.args())
        err, fed = _drive_until_error(be, sim, ex)
        assert err is not None and fed <= 5, "no sharded update within the first messages (%d fed)" % fed
        assert ex.calls == 1 and ex.aborts == 0
        if how == "poisoned_peer":
            assert "lvk status 2:" in str(err) and "mask 0x2" in str(err), str(err)
            assert ex.sizes and ex.sizes[0] >= 512
        else:
            assert "lvk status 2:" in str(err) and "the exchange callback failed" in str(err), str(err)
        be.close()
        _assert_context_still_runs_the_unsharded_filter(ctx, gpu_ctx)
    finally:
        ctx.close()


class _Lockstep:
    """All-gather among the threads of one process: every rank puts its block into a shared slot, a barrier, every rank reads all
    slots, a second barrier (no slot is overwritten before all have read it).  A broken barrier - a peer that failed, or the
    timeout - makes every callback return an error, so a failure in one rank ends the others."""

    def __init__(self, world):
        self.world = world; self.barrier = threading.Barrier(world); self.slots = [None] * world
        self.ks = []                                              # per exchange: every rank's k, from the headers rank 0 received

    def rank(self, ctx, rank):
        return _LockstepRank(self, ctx, rank)


class _LockstepRank:
    def __init__(self, shared, ctx, rank):
        from larvio_amd import sharding
        self.sh, self.ctx, self.rank_ = shared, ctx, rank
        self.calls = 0
        self._cb = sharding.EXCHANGE_FN(self._call)

    def _call(self, user, d_send, d_recv, nbytes, stream):
        from larvio_amd._lib import lib
        sh = self.sh
        try:
            if nbytes == 0:                                       # abort (lvk_exchange_fn contract): make the peers' exchange fail
                sh.barrier.abort()
                return 2
            L = lib()
            self.ctx.sync()
            mine = np.empty(nbytes, np.uint8)
            self.ctx.check(L.lvk_memcpy_d2h(self.ctx.h, mine.ctypes.data_as(C.c_void_p), C.c_void_p(d_send), nbytes))
            sh.slots[self.rank_] = mine
            sh.barrier.wait(_WAIT)
            parts = list(sh.slots)
            if any(p is None or p.size != nbytes for p in parts):
                raise RuntimeError("the ranks disagree about the block size: %s" % [None if p is None else p.size for p in parts])
            allb = np.concatenate(parts)
            self.ctx.check(L.lvk_memcpy_h2d(self.ctx.h, C.c_void_p(d_recv), allb.ctypes.data_as(C.c_void_p), allb.nbytes))
            self.ctx.sync()
            if self.rank_ == 0:
                sh.ks.append([_header_k(p) for p in parts])
            sh.barrier.wait(_WAIT)
            self.calls += 1
            return 0
        except threading.BrokenBarrierError:
            return 2
        except Exception as exc:                                  # never let an exception cross the C frame
            print("lock-step exchange failed on rank %d: %r" % (self.rank_, exc))
            sh.barrier.abort()
            return 2

    def args(self):
        return self.rank_, self.sh.world, C.cast(self._cb, C.c_void_p), None, self


@pytest.mark.parametrize("world", [3, 4])
def test_worlds_three_and_four_in_lock_step_are_bit_identical_and_match_the_unsharded_filter(gpu_ctx, world):
    """one thread, one Context(0) and one filter per rank on the same simulated messages: identical bits on every rank, the
    unsharded filter's ids and counters, 1e-6 of its state and covariance (the two-rank test's tolerance: another reduction tree,
    same information), one exchange per sharded update, every rank stacked rows, and the ranks' k differed (k < k_max occurred)"""
    import larvio_amd
    from larvio_amd import larvio as lv
    from larvio_amd._lib import lib
    sim = _small_sim()
    n_ref, s_ref, P_ref, cid_ref, fid_ref, cnt_ref = _small_ref(gpu_ctx)
    assert n_ref >= 10
    lib(); lv._L()                                                # bind the signatures before the threads start
    shared = _Lockstep(world); out = [None] * world

    def worker(rank):
        ctx = None
        try:
            ctx = larvio_amd.Context(0)
            be = larvio_amd.LarVio(sim["cfg"], ctx); assert be.initialize()
            ex = shared.rank(ctx, rank)
            be.set_shard(*ex.args())
            n, s, P, cid, fid, cnt = _run(be, sim)
            out[rank] = (n, {k: np.array(v) for k, v in s.items()}, P, cid, fid, cnt, be.shard_stats(), ex.calls)
            be.close()
        except BaseException:
            import traceback
            out[rank] = traceback.format_exc()
            shared.barrier.abort()                                # the others' next exchange fails instead of waiting
        finally:
            if ctx is not None:
                ctx.close()

    threads = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(4 * _WAIT)
        assert not t.is_alive(), "a rank did not finish"
    for r in range(world):
        assert isinstance(out[r], tuple), "rank %d:\n%s" % (r, out[r])
    a = out[0]
    for r in range(1, world):
        b = out[r]
        assert a[0] == b[0]
        for k in a[1]:
            assert np.array_equal(a[1][k].view(np.uint64), b[1][k].view(np.uint64)), (r, k)   # replicas: identical bits
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5], r
    rel = lambda x, y: float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300))
    worst = max(rel(a[1][k], s_ref[k]) for k in ("q", "v", "p", "bg", "ba", "R_b2c", "t_c_b"))
    print("lock step x%d: updates %d, worst rel vs unsharded %.3g / %.3g, stats %s, k per exchange %s" % (world, a[0], worst, rel(a[2], P_ref), [o[6] for o in out], shared.ks))
    assert a[0] == n_ref and np.array_equal(a[3], cid_ref) and np.array_equal(a[4], fid_ref)
    # the filter's decisions; "triangulations" counts kernel requests, which the sharded path (results read back before the rows are
    # laid out) and the unsharded one (triangulations consumed on the device) issue differently - it is compared across ranks above
    assert set(cnt_ref) - {"triangulations"} >= {"hybrid", "msckf", "gated_in", "gated_out", "map"}
    for k in set(cnt_ref) - {"triangulations"}:
        assert a[5][k] == cnt_ref[k], (k, a[5], cnt_ref)
    assert worst < 1e-6 and rel(a[2], P_ref) < 1e-6, (worst, rel(a[2], P_ref))
    for r in range(world):
        st = out[r][6]
        assert st["sharded_updates"] >= 5 and st["exchanges"] == st["sharded_updates"] == out[r][7] and st["bytes_sent"] > 0, (r, st)
        assert st["rows_stacked"] > 0, (r, st)
    assert len(shared.ks) == a[6]["exchanges"]
    assert any(len(set(ks)) > 1 for ks in shared.ks), "every exchange had the same k on every rank"
    assert all(any(ks[r] > 0 for ks in shared.ks) for r in range(world))
