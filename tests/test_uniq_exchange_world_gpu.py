"""uniq's hash-range exchange at world > 1 ON THE DEVICE KERNELS (run with -m gpu): circkit_amd/uniq.py::first_seen with a
DeviceTable per rank, the ranks being threads of this process and the collectives tests/loopback_dist.py -- one GPU, no RCCL.
Rank r of a threaded world owns ctx r of a module-wide pool of eight ctxs on device 0, a torch stream of its own and a
DeviceTable, so up to eight tables are live and their kernels may overlap.  What no other test runs: the counts the partition
kernel returns cut the rows it wrote, an owner's table folds interleaved global indices of several senders (the smallest often
NOT the asker's), the ~0 key crosses ranks, shards and owners are empty, the answers return through the third all-to-all into
the gather, and DeviceTable rebinds eight live ctxs.

Every comparison is per record against tests/uniq_keys.py's expected_first_seen over the JOINED shards (the plain restatement
"smallest global index per key"), never against another GPU result; keep is compared against `expected == own index`.

The shard shapes (SIZES, world_job) are shared with tests/test_loopback_dist_cpu.py, which runs them through the same loopback
with the NumPy tables of tests/test_uniq_sharded.py.  Descending bases (rank r holds LOWER global indices than rank r - 1)
separate "smallest global index" from "first to arrive".

Wall time of this file on one MI355X: 17 tests in 3.6 s as pytest counts it, most of it imports and the first use of the device;
the pool of eight ctxs and eight streams takes 0.25 s; the slowest test takes 0.6 s (the pairs / all-gather branches at world 2,
the first to run torch's sort and bincount), every other one 0.35 s or less.

What the file was seen to catch, on scratch builds of the library with one slip each (both in bounds):
  uniq_fold without its atomicMin on a key that is present    14 of 17 fail: every world, branch and base order, the compact, the
  (whoever claims a key keeps it: "first to arrive")          bench's job, both phased worlds (the ~0 key's runs and the damage
                                                              controls pass, as they must)
  the ~0 key's value stored plainly instead of atomicMin       8 of 17 fail: world 8 in both orders, both other branches, the
  (the last writer wins)                                      one-key run on ~0, the compact, both phased worlds"""
import functools
import time

import numpy as np
import pytest

from tests import loopback_dist as LD
from tests import uniq_keys as K

pytestmark = pytest.mark.gpu

EMPTY = K.EMPTY
BASE = 7_000_000_000                                    # beyond 2^32: an index kept in 32 bits somewhere shows
ORDERS = ("ascending", "descending")
# both sides of the scatter kernel's 1024-key chunk, one record, empty shards (in the middle at world 3, rank 0 at world 8)
SIZES = {2: [5000, 1025], 3: [4097, 0, 1023], 8: [0, 1, 1023, 1025, 5000, 40000, 4097, 256]}
SENT64, SENT32, PAD = 0x5E5E5E5E5E5E5E5E, 0x5E5E5E5E, 8


# ---- the job: shards, bases and the restatement's answer (NumPy only; also used by the CPU test of the loopback) ---------------
class Job:
    """shards[r]: uint64 keys of rank r; bases[r]: global index of its record 0; exp: expected first-seen of every record of the
    job, the shards joined in rank order; index: the records' own global indices, joined the same way"""

    def __init__(self, shards, order):
        assert order in ORDERS
        self.world = len(shards)
        self.shards = [np.ascontiguousarray(s, dtype=np.uint64) for s in shards]
        sizes = np.array([len(s) for s in self.shards], dtype=np.int64)
        self.cuts = np.r_[0, np.cumsum(sizes)].astype(np.int64)
        total = int(self.cuts[-1])
        self.bases = BASE + (self.cuts[:-1] if order == "ascending" else total - self.cuts[1:])
        self.all_h = np.concatenate(self.shards)
        self.index = np.concatenate([b + np.arange(n, dtype=np.int64) for b, n in zip(self.bases, sizes)])
        self.rank_of = np.repeat(np.arange(self.world), sizes)
        self.exp = K.expected_first_seen(self.all_h, self.index)
        for a in self.shards + [self.all_h, self.index, self.exp]:
            a.setflags(write=False)                                 # computed once, shared, left unchanged

    def expected(self, rank):
        return self.exp[self.cuts[rank]:self.cuts[rank + 1]]

    def own(self, rank):
        return self.index[self.cuts[rank]:self.cuts[rank + 1]]

    def cross_fraction(self):
        """share of the job's records whose first occurrence lives on another rank"""
        pos_of = np.argsort(self.index)                             # the indices are BASE .. BASE + total - 1, each once
        first_rank = self.rank_of[pos_of[self.exp - BASE]]
        return float((first_rank != self.rank_of).mean())


@functools.lru_cache(maxsize=None)
def world_job(world, order):
    """Every key about four times across the job; 2 * world records of the ~0 key at random positions, one of them in every
    shard that has records (six random positions at world 3 all fall into the 4097-record shard one time in four)."""
    sizes = SIZES[world]
    rng = np.random.default_rng(1000 + world)
    total = sum(sizes)
    pool = K.random_keys(rng, total // 4)
    h = pool[rng.integers(0, len(pool), size=total)]
    cuts = np.r_[0, np.cumsum(sizes)]
    spread = np.array([cuts[r] + rng.integers(0, sizes[r]) for r in range(world) if sizes[r]])
    others = rng.choice(np.setdiff1d(np.arange(total), spread), size=2 * world - len(spread), replace=False)
    h[np.concatenate([spread, others])] = EMPTY
    assert int((h == EMPTY).sum()) == 2 * world
    return Job([h[cuts[r]:cuts[r + 1]] for r in range(world)], order)


def check_generator(job):
    """The three conditions on a world_job, from the restatement alone (nothing here has seen a GPU), and the ~0 key's spread."""
    assert job.cross_fraction() >= 0.10, job.cross_fraction()
    assert int((job.exp == job.index).sum()) == len(np.unique(job.all_h))
    assert np.all(np.bincount(K.owner(job.all_h, job.world).astype(np.int64), minlength=job.world) > 0)
    assert len(np.unique(job.rank_of[job.all_h == EMPTY])) >= 2


def mismatches(job, results):
    """records of the job whose first-seen index or keep flag differs from the restatement; results[r] = (fs, keep, ...)"""
    bad = 0
    for rank, res in enumerate(results):
        fs, keep = res[0], res[1]
        exp = job.expected(rank)
        assert fs.shape == exp.shape and keep.shape == exp.shape, (rank, fs.shape, keep.shape, exp.shape)
        bad += int(((fs != exp) | (keep != (exp == job.own(rank)))).sum())
    return bad


# ---- the device side -----------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    """a NumPy array (uint64 as int64) on the device, copied on the caller's current stream"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(_dev())


def _u64(t, k=None):
    a = t.cpu().numpy().view(np.uint64)
    return a if k is None else a[:k]


class Pool:
    def __init__(self, n):
        import torch
        import circkit_amd
        t0 = time.perf_counter()
        self.ctxs = [circkit_amd.Context(0) for _ in range(n)]
        self.streams = [torch.cuda.Stream(device=_dev()) for _ in range(n)]
        torch.cuda.synchronize()
        self.seconds = time.perf_counter() - t0
        print("pool of %d ctxs and streams: %.3f s" % (n, self.seconds))

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture(scope="module")
def pool():
    import torch
    p = Pool(8)
    yield p
    torch.cuda.synchronize()
    p.close()


def run_world(monkeypatch, pool, job, exchange="partition", wrap=None, damage=None, after=None):
    """uniq.first_seen in one thread per rank: rank r on ctx r, its own stream, its own DeviceTable; table.check() behind it.
    Returns (the loopback world, [(fs, keep[, after(rank, ctx, fs, keep)])] per rank) with fs and keep on the host."""
    import torch
    from circkit_amd import uniq
    w = LD.install(monkeypatch, job.world, damage)

    def rank_fn(rank):
        ctx = pool.ctxs[rank]
        with torch.cuda.stream(pool.streams[rank]):
            table = uniq.DeviceTable(ctx)
            d_hash = _to(job.shards[rank])
            fs, keep = uniq.first_seen(wrap(table) if wrap else table, d_hash, base_index=int(job.bases[rank]), exchange=exchange)
            table.check()
            out = (fs.cpu().numpy().view(np.int64), keep.cpu().numpy().astype(bool))
            return out + ((after(rank, ctx, fs, keep),) if after else ())

    return w, w.run(rank_fn)


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_partition_exchange_at_world_n(monkeypatch, pool, world, order):
    """The default branch of a multi-GPU job: partition -> all_to_all of the counts -> all_to_all of the owner groups -> reset
    sized for the received rows -> insert_rows / lookup_rows on rows of several senders -> all_to_all of the answers ->
    gather.  Exactly three all_to_all_single calls per rank and no all_gather: the device-rows branch, not the torch-op one."""
    job = world_job(world, order)
    check_generator(job)
    w, results = run_world(monkeypatch, pool, job)
    assert w.all_to_all_calls == [3] * world and w.all_gather_calls == [0] * world
    assert mismatches(job, results) == 0
    assert sum(int(r[1].sum()) for r in results) == len(np.unique(job.all_h))


class PairsOnly:
    """a DeviceTable without `partition` (and `resolve`): first_seen takes the argsort / insert_pairs / lookup branch"""

    def __init__(self, table):
        self.reset, self.insert, self.insert_pairs, self.lookup = table.reset, table.insert, table.insert_pairs, table.lookup


@pytest.mark.parametrize("world", [2, 8])
def test_pairs_and_allgather_branches_at_world_n(monkeypatch, pool, world):
    """The two other branches against the same expectation, both base orders: the torch-op exchange (argsort, bincount, three
    all_to_all, insert_pairs / lookup on pairs of several senders) and exchange="allgather" (two all_gather, one insert per
    rank with that rank's base, shards padded to the largest)."""
    for order in ORDERS:
        job = world_job(world, order)
        w, results = run_world(monkeypatch, pool, job, wrap=PairsOnly)
        assert w.all_to_all_calls == [3] * world and w.all_gather_calls == [0] * world
        assert mismatches(job, results) == 0, ("pairs", order)
        w, results = run_world(monkeypatch, pool, job, exchange="allgather")
        assert w.all_to_all_calls == [0] * world and w.all_gather_calls == [2] * world
        assert mismatches(job, results) == 0, ("allgather", order)


@pytest.mark.parametrize("case", ["one_owner", "one_key", "the_empty_key"])
def test_one_owner_and_one_key(monkeypatch, pool, case):
    """World 8, descending bases.  one_owner: every key belongs to rank 7, so seven owners receive nothing and take the
    reset(1) / lookup_rows path on zero rows, and seven ranks get every answer from one peer.  one_key / the_empty_key: every
    record of every rank carries one single key (an ordinary one; ~0), and 8 x 4096 records resolve to one global index, the
    first record of rank 7."""
    world = 8
    rng = np.random.default_rng(808)
    if case == "one_owner":
        keys = K.owned_by(rng, 1700, 7, world)
        job = Job([keys[rng.integers(0, len(keys), size=n)] for n in SIZES[world]], "descending")
        assert np.bincount(K.owner(job.all_h, world).astype(np.int64), minlength=world).tolist()[:7] == [0] * 7
        assert job.cross_fraction() >= 0.10
    else:
        key = EMPTY if case == "the_empty_key" else K.random_keys(rng, 1)[0]
        job = Job([np.full(4096, key, dtype=np.uint64)] * world, "descending")
        assert np.all(job.exp == BASE) and int(job.bases[7]) == BASE
    w, results = run_world(monkeypatch, pool, job)
    assert w.all_to_all_calls == [3] * world
    assert mismatches(job, results) == 0
    assert sum(int(r[1].sum()) for r in results) == len(np.unique(job.all_h))


def test_answers_feed_the_compact_with_a_base(monkeypatch, pool):
    """World 3, descending bases: every rank packs a payload of 1..40 random bytes per record with circkit_uniq_compact_device,
    d_first_seen being what the exchange's gather wrote and base_index the shard's base, both dup outputs asked for.  Each
    rank's batch must be uniq_compact_ref.compact's for the restatement's first-seen of that shard; dup_first holds indices of
    OTHER ranks' records; over all ranks the kept records are exactly the job's distinct keys."""
    import torch
    from tests import monomers_sets as MS
    from tests import uniq_compact_ref as UR
    guard, canary, canary64 = 64, 0x3F, 0x2D2D2D2D2D2D2D2D
    job = world_job(3, "descending")
    rng = np.random.default_rng(33)
    payload = [MS.batch(rng, rng.integers(1, 41, size=len(s))) for s in job.shards]

    def compact(rank, ctx, fs, keep):
        data, offs = payload[rank]
        n, nb = len(offs) - 1, len(data)
        d_raw = _to(np.concatenate([np.full(guard, 0x4E, dtype=np.uint8), data, np.full(guard, 0x4E, dtype=np.uint8)]))
        d_offs = _to(offs)
        d_out = torch.full((nb + guard,), canary, dtype=torch.uint8, device=_dev())
        full = lambda k: torch.full((k + guard,), canary64, dtype=torch.int64, device=_dev())     # noqa: E731
        d_out_off, d_out_src, d_dsrc, d_dfirst = full(n + 1), full(n), full(n), full(n)
        ctx.uniq_compact_device(d_raw[guard:], d_offs, n, fs, d_out, d_out_off, d_out_src, base_index=int(job.bases[rank]),
                                d_dup_src=d_dsrc, d_dup_first=d_dfirst)
        m, nbytes = ctx.uniq_compact_status()
        assert 0 <= m <= n and 0 <= nbytes <= nb
        out = d_out.cpu().numpy()
        assert (out[nbytes:] == canary).all() and (_u64(d_out_off)[m + 1:] == canary64).all() and (_u64(d_out_src)[m:] == canary64).all()
        assert (_u64(d_dsrc)[n - m:] == canary64).all() and (_u64(d_dfirst)[n - m:] == canary64).all()
        return out[:nbytes], _u64(d_out_off, m + 1), _u64(d_out_src, m), _u64(d_dsrc, n - m), _u64(d_dfirst, n - m)

    w, results = run_world(monkeypatch, pool, job, after=compact)
    assert mismatches(job, results) == 0
    kept, foreign = [], 0
    for rank, (_, _, got) in enumerate(results):
        data, offs = payload[rank]
        base, n = int(job.bases[rank]), len(offs) - 1
        exp = UR.compact(data, offs, job.expected(rank).astype(np.uint64), base)
        UR.assert_equal(got, exp, "rank %d" % rank)
        kept.append(job.shards[rank][got[2].astype(np.int64)])
        foreign += int(((got[4] < np.uint64(base)) | (got[4] >= np.uint64(base + n))).sum())
    assert foreign > 0.10 * len(job.all_h)                          # first occurrences on other ranks, as indices of theirs
    assert np.array_equal(np.sort(np.concatenate(kept)), np.unique(job.all_h))


def test_bench_job_check_at_world_8(monkeypatch, pool):
    """bench.py --workload uniq --gpus 8 at reduced size (4096 records of 100 b per rank): the device fill, duplicates planted
    from base records of ALL ranks, hashes from the canonicalize call's fused XXH3, first_seen through the loopback, then the
    check the bench exits non-zero on."""
    import torch
    from circkit_amd import uniq, workloads as W
    world, n, length = 8, 4096, 100
    w = LD.install(monkeypatch, world)
    dev = _dev()

    def rank_fn(rank):
        ctx = pool.ctxs[rank]
        with torch.cuda.stream(pool.streams[rank]):
            table = uniq.DeviceTable(ctx)                           # (binds the ctx to this rank's stream)

            def fill(seed, first_base, n_bases):
                buf = torch.empty(n_bases + 64, dtype=torch.uint8, device=dev)
                ctx.synth_fill_device(seed, first_base, n_bases, buf)
                return buf
            d_bytes, d_off = W.fixed_length(ctx, dev, n, length, 42, rank * n)
            W.plant_job_duplicates(fill, d_bytes, n, length, dev, rank, world)
            d_hash = torch.empty(n, dtype=torch.int64, device=dev)
            ctx.canonicalize_batch_device(d_bytes, d_off, n, out_xxh3=d_hash)
            fs, keep = uniq.first_seen(table, d_hash, base_index=rank * n)
            table.check()
            wrong, cross, distinct, _ = W.job_check(fs, keep, n, length, world, rank, dev)
            return wrong, cross, distinct, int(keep.sum())

    res = w.run(rank_fn)
    assert w.all_to_all_calls == [3] * world
    assert [r[0] for r in res] == [0] * world, res
    assert all(r[2] == world * (n // 2) for r in res)
    assert sum(r[3] for r in res) == world * (n // 2)
    assert sum(r[1] for r in res) > world * n // 4


def _status(ctx):
    import ctypes
    n = ctypes.c_uint32(0xDEAD)
    rc = ctx._lib.circkit_uniq_status(ctx._h, ctypes.byref(n))
    return rc, n.value


@pytest.mark.parametrize("world", [63, 64])
def test_phased_exchange_between_two_ctxs(pool, world):
    """The C-ABI contract (include/circkit.h, "The device steps of the multi-GPU exchange") at the two worlds next to the
    prefix sum's width, without threads and without uniq.py: one shard per rank, 0..3000 records each from a seeded draw, two
    of them empty, descending bases.  Every shard is partitioned on ctx A with sentinels round d_rows, d_slot and d_counts;
    for each owner the shards' groups are cut out by the counts THE KERNEL returned and joined in sender order (the all-to-all,
    done by slicing; a group starts on a row, i.e. a multiple of 16 bytes); ctx B resets for the rows it got, folds them, and
    answers; the answers are cut back per sender into each sender's row order and gathered on A."""
    import torch
    dev = _dev()
    rng = np.random.default_rng(6300 + world)
    sizes = rng.integers(0, 3001, size=world)
    sizes[[5, 40]] = 0
    total = int(sizes.sum())
    keys = K.random_keys(rng, total // 4)
    h = keys[rng.integers(0, len(keys), size=total)]
    h[rng.choice(total, size=2 * world, replace=False)] = EMPTY
    cuts = np.r_[0, np.cumsum(sizes)]
    job = Job([h[cuts[r]:cuts[r + 1]] for r in range(world)], "descending")
    assert job.cross_fraction() >= 0.10 and int((sizes == 0).sum()) >= 2
    a, b = pool.ctxs[0], pool.ctxs[1]
    for c in (a, b):
        c.set_stream(torch.cuda.current_stream().cuda_stream)

    # phase 1: every shard partitioned on A
    parts = []
    for s in range(world):
        n = int(sizes[s])
        rows_buf = torch.full(((n + 2 * PAD) * 2,), SENT64, dtype=torch.int64, device=dev)
        slot_buf = torch.full((n + 2 * PAD,), SENT32, dtype=torch.int32, device=dev)
        counts_buf = torch.full((world + PAD,), SENT64, dtype=torch.int64, device=dev)
        rows, slot = rows_buf[2 * PAD:2 * PAD + 2 * n], slot_buf[PAD:PAD + n]
        assert rows_buf.data_ptr() % 16 == 0
        a.uniq_partition_device(_to(job.shards[s]), n, int(job.bases[s]), world, rows if n else None, counts_buf, slot if n else None)
        cb = counts_buf.cpu().numpy()
        counts = cb[:world].copy()
        assert np.all(cb[world:] == SENT64)
        assert np.array_equal(counts, np.bincount(K.owner(job.shards[s], world).astype(np.int64), minlength=world)), s
        rb, sb = rows_buf.cpu().numpy(), slot_buf.cpu().numpy()
        assert np.all(rb[:2 * PAD] == SENT64) and np.all(rb[2 * PAD + 2 * n:] == SENT64), s
        assert np.all(sb[:PAD] == SENT32) and np.all(sb[PAD + n:] == SENT32), s
        parts.append((rows.view(n, 2), slot, counts, np.r_[0, np.cumsum(counts)]))

    # phase 2: every owner's table on B
    answers = []
    for o in range(world):
        groups = [rows[starts[o]:starts[o + 1]] for rows, _, _, starts in parts]
        assert all(g.data_ptr() % 16 == 0 for g in groups if g.shape[0])
        recv = torch.cat(groups)
        n_o = recv.shape[0]
        assert n_o == sum(int(p[2][o]) for p in parts) and recv.data_ptr() % 16 == 0
        b.uniq_reset(max(n_o, 1))
        b.uniq_insert_rows_device(recv if n_o else None, n_o)
        ans = torch.full((n_o + PAD,), SENT64, dtype=torch.int64, device=dev)
        b.uniq_lookup_rows_device(recv if n_o else None, n_o, ans)
        assert _status(b) == (0, 0), o
        answers.append(ans)
    assert all(bool((ans[-PAD:] == SENT64).all()) for ans in answers)

    # phase 3: the answers back to their senders, in each sender's row order, and the gather on A
    sent = np.zeros(world, dtype=np.int64)                          # rows of each owner's answers handed back so far
    bad = 0
    for s, (_, slot, counts, _) in enumerate(parts):
        n = int(sizes[s])
        back = torch.cat([answers[o][sent[o]:sent[o] + counts[o]] for o in range(world)])
        sent += counts
        assert back.shape[0] == n
        fs = torch.full((n + PAD,), SENT64, dtype=torch.int64, device=dev)
        keep = torch.full((n + PAD,), 7, dtype=torch.uint8, device=dev)
        a.uniq_gather_device(back if n else None, slot if n else None, n, int(job.bases[s]), fs, keep)
        fs, keep = fs.cpu().numpy(), keep.cpu().numpy()
        assert np.all(fs[n:] == SENT64) and np.all(keep[n:] == 7)
        exp = job.expected(s)
        bad += int(((fs[:n] != exp) | (keep[:n] != (exp == job.own(s)))).sum())
    assert bad == 0
    assert _status(a) == (0, 0)


@pytest.mark.parametrize("damage", [("roll", 3), ("own", 2)], ids=["answers_rolled_by_one", "only_the_own_slice_arrives"])
def test_damaged_exchanges_are_caught(monkeypatch, pool, damage):
    """Negative controls with the real kernels at world 3: the answers of the third all-to-all rolled by one row, and a second
    all-to-all in which every rank receives only its own slice (its peers' rows arrive as zeros).  Only data is wrong -- every
    size and pointer is the undamaged run's -- and the comparison must say so."""
    job = world_job(3, "descending")
    w, results = run_world(monkeypatch, pool, job, damage=LD.Damage(*damage))
    assert w.all_to_all_calls == [3] * 3
    assert mismatches(job, results) > 0
