"""The uniq first-seen table on crafted keys (run with -m gpu): the paths that well-mixed keys in a correctly sized table never
reach.  Table overflow (counted, reported, survivable), probe chains that wrap at the last slot, the LDS bucket boundary of the
bucketed resolve (3072 / 3073 rows), one key a million times against the plain peek ahead of the atomics, the streaming table's
growth on both sides of its condition, the partition kernels at their chunk edges, and the refusals.

Every comparison is exact: every record and every key against tests/uniq_keys.py's expected_first_seen, the plain restatement
"smallest index per key".  The generators there aim the input at the slot / bucket / owner functions; no expected value
depends on them.  One ctx per test, closed at the end.

Wall time of this file on one MI355X: 48 tests in about 3.5 s (1.7 s of it the first ctx; no test above 0.2 s).

What the file was seen to catch, on scratch builds of the library with one slip each (all of them in bounds):
  `++probes > mask` -> `>= mask` (fold and lookups)          test_a_full_circle_of_probes_reaches_the_last_free_slot fails
                                                              (random keys fill the table either way: the overflow test passes)
  no wrap in uniq_fold / uniq_fold_local (the end = full)    the full-circle test, every case of the wrapping clusters, shard (b)
  the fallback lookup without its `only_if` flag             shards (a) and (c) of the bucket boundary ((b) sets the flag anyway)
  `cnt > BKT_MAX` -> `>=`                                     nothing, as expected: the answers are the same on either path
A build without the `& mask` at all would probe past the table's end; that one is not to be run on a GPU."""
import ctypes

import numpy as np
import pytest

from tests import uniq_keys as K

pytestmark = pytest.mark.gpu

EMPTY = K.EMPTY
INVALID_ARG, OOM = -1, -5
BASE = 7_000_000_000                                    # beyond 2^32: an index kept in 32 bits somewhere shows


@pytest.fixture
def ctx():
    import torch
    import circkit_amd
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)           # ordered with the torch copies around the calls
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _insert(ctx, path, h, idx):
    """folds the (key, index) records into the ctx table through one of its three insert entries"""
    n = len(h)
    if path == "device":                                            # indices base + i
        assert np.array_equal(idx, idx[0] + np.arange(n, dtype=np.uint64))
        ctx.uniq_insert_device(_dev(h), n, int(idx[0]))
    elif path == "pairs":
        ctx.uniq_insert_pairs_device(_dev(h), _dev(idx), n)
    else:
        ctx.uniq_insert_rows_device(_dev(np.stack([h, idx], axis=1)), n)


def _lookup(ctx, path, h):
    import torch
    n = len(h)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int64, device=torch.device("cuda", 0))
    if path == "rows":
        ctx.uniq_lookup_rows_device(_dev(np.stack([h, np.full(n, 123, dtype=np.uint64)], axis=1)), n, out)
    else:
        ctx.uniq_lookup_device(_dev(h), n, out)
    return _u64(out)


def _indices(rng, path, n):
    """global indices of n records: base + i where the entry takes no others, else shuffled"""
    i = np.arange(n, dtype=np.uint64) + np.uint64(BASE)
    return i if path in ("device", "resolve", "host") else rng.permutation(i)


def _status(ctx):
    n = ctypes.c_uint32(0xDEAD)
    rc = ctx._lib.circkit_uniq_status(ctx._h, ctypes.byref(n))
    return rc, n.value


# ---- 1. overflow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["device", "pairs", "rows"])
def test_overflow_is_counted_reported_and_survivable(ctx, path):
    """uniq_reset(10) gives the documented minimum of 1024 slots; 2000 distinct keys and the ~0 key, each twice, go in.  The
    table fills completely: exactly 1024 ordinary keys are answered, with the right value, and the ~0 key (a slot of its
    own) always; every record of another key -- and 100 keys never inserted, after a full circle of probes -- reads ~0;
    circkit_uniq_status reports CIRCKIT_ERR_OOM and counts exactly the records whose key found no slot (WHICH keys win a slot
    depends on scheduling, how many does not).  A defined error path, no device fault.  After uniq_reset(4002) the same
    insert is clean."""
    import circkit_amd
    rng = np.random.default_rng(101)
    pool = K.random_keys(rng, 2100)
    keys, never = np.append(pool[:2000], EMPTY), pool[2000:]
    h = rng.permutation(np.concatenate([keys, keys]))
    n = len(h)
    assert n == 4002
    idx = _indices(rng, path, n)
    exp = K.expected_first_seen(h, idx)

    ctx.uniq_reset(10)
    _insert(ctx, path, h, idx)
    got = _lookup(ctx, path, h)
    answered = got != EMPTY
    won, lost = np.unique(h[answered]), np.unique(h[~answered])
    assert len(np.intersect1d(won, lost)) == 0                      # both records of a key read alike
    assert EMPTY in won
    assert len(won) - 1 == 1024, len(won) - 1                       # the table is full, to the last slot
    assert np.array_equal(got[answered], exp[answered])
    assert np.all(_lookup(ctx, path, never) == EMPTY)
    rc, n_overflowed = _status(ctx)
    assert rc == OOM
    assert n_overflowed == int((~answered).sum()), (n_overflowed, int((~answered).sum()))
    assert ctx.uniq_overflowed() == n_overflowed
    with pytest.raises(circkit_amd.CirckitError) as e:
        ctx.uniq_status()
    assert e.value.code == OOM and "overflow" in str(e.value)

    ctx.uniq_reset(n)
    _insert(ctx, path, h, idx)
    got = _lookup(ctx, path, h)
    assert _status(ctx) == (0, 0)
    assert ctx.uniq_overflowed() == 0
    ctx.uniq_status()
    assert np.array_equal(got, exp)
    assert np.all(_lookup(ctx, path, never) == EMPTY)


@pytest.mark.parametrize("path", ["device", "pairs", "rows"])
def test_a_full_circle_of_probes_reaches_the_last_free_slot(ctx, path):
    """Random keys fill a table whatever the probe limit is, one short included.  Here 1024 keys that all start at the same
    slot go into the 1024-slot table, each twice, with the ~0 key beside them: the table is exactly full, and the key that
    comes last finds its slot only with the 1024th probe, a full circle.  No overflow; every record right; absent keys of
    the same chain read ~0 after a full circle.  Five more such keys then overflow, twice each: counted as 10, they read ~0
    and nothing else changes."""
    rng = np.random.default_rng(111)
    pool = K.clustered(rng, 1024 + 5 + 20)
    keys, more, never = np.append(pool[:1024], EMPTY), pool[1024:1029], pool[1029:]
    h = rng.permutation(np.concatenate([keys, keys]))
    idx = _indices(rng, path, len(h))
    exp = K.expected_first_seen(h, idx)
    ctx.uniq_reset(10)
    _insert(ctx, path, h, idx)
    got = _lookup(ctx, path, h)
    assert _status(ctx) == (0, 0)
    assert np.array_equal(got, exp), int((got != exp).sum())
    assert np.all(_lookup(ctx, path, never) == EMPTY)
    h2 = np.concatenate([more, more])
    _insert(ctx, path, h2, np.arange(len(h2), dtype=np.uint64) + np.uint64(5))      # (smaller indices: they would win if they got in)
    assert np.all(_lookup(ctx, path, h2) == EMPTY)
    assert np.array_equal(_lookup(ctx, path, h), exp)
    assert _status(ctx) == (OOM, 10)


# ---- 2. clusters that wrap -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["distinct", "tripled"])
@pytest.mark.parametrize("path", ["device", "pairs", "rows", "resolve", "host"])
def test_clusters_that_wrap_at_the_last_slot(path, form):
    """700 keys that all start probing three slots before the end of the table, and the ~0 key: in the 1024-slot table that
    expected_keys = 701 gives (70 % rule) they are one probe chain over slots 1021, 1022, 1023, 0 .. 696, so almost every
    insert and lookup steps from the last slot to slot 0 -- right in front of the ~0 key's own slot [1024] -- and walks
    hundreds of slots.  The resolve call sizes its table for the records (1024 or 4096 slots) and the host form takes at
    least 65536: the keys cluster at the end of every power-of-two table up to 2^24 slots."""
    import torch
    import circkit_amd
    rng = np.random.default_rng(202)
    keys = np.append(K.clustered(rng, 700), EMPTY)
    h = rng.permutation(np.tile(keys, 3 if form == "tripled" else 1))
    n = len(h)
    idx = _indices(rng, path, n)
    exp = K.expected_first_seen(h, idx)
    never = K.clustered(rng, 800)
    never = never[~np.isin(never, keys)][:50]                       # absent keys of the same chain: the lookup walks it to its end
    c = circkit_amd.Context(0)
    try:
        if path == "host":
            got = c.uniq_first_seen(h, BASE)
        elif path == "resolve":
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            fs = torch.full((n,), -1, dtype=torch.int64, device=torch.device("cuda", 0))
            keep = torch.full((n,), 7, dtype=torch.uint8, device=torch.device("cuda", 0))
            c.uniq_resolve_device(_dev(h), n, BASE, fs, keep)
            got = _u64(fs)
            assert np.array_equal(keep.cpu().numpy(), (exp == idx).astype(np.uint8))
        else:
            c.set_stream(torch.cuda.current_stream().cuda_stream)
            c.uniq_reset(len(keys))
            _insert(c, path, h, idx)
            got = _lookup(c, path, h)
            assert np.all(_lookup(c, path, never) == EMPTY)
        assert _status(c) == (0, 0)
        assert np.array_equal(got, exp), int((got != exp).sum())
    finally:
        c.close()


# ---- 3. the LDS bucket boundary ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shard", ["a_3072_rows", "b_3073_rows", "c_3072_rows_500_empty_keys"])
def test_lds_bucket_boundary_and_lds_clusters(ctx, shard):
    """A shard of exactly 2^19 records is resolved in 256 buckets by the top 8 bits (the sizing rule).  (a) one bucket holds
    exactly 3072 rows, the most that is resolved in LDS: 3072 distinct clustered keys, the longest chain the 4096-slot LDS
    table can see, wrapping at slot 4095; (b) the same with 3073 rows: the whole shard takes the HBM fallback; (c) bucket 255
    holds 3072 rows of which 500 are the ~0 key.  The rest of each shard is random with ~3x duplication.  Results must be
    right on both sides of the boundary; WHICH path ran is not observable here -- tests/test_uniq_keys_cpu.py checks that
    the inputs have exactly these row counts."""
    import torch
    bucket, rows, empty_rows = {"a": (0xAB, 3072, 0), "b": (0xAB, 3073, 0), "c": (255, 3072, 500)}[shard[0]]
    n = 1 << 19
    h = K.bucket_shard(np.random.default_rng(3), n, bucket, rows, empty_rows)
    exp = K.expected_first_seen(h)
    exp_keep = (exp == np.arange(n)).astype(np.uint8)
    d_h = _dev(h)
    dev = torch.device("cuda", 0)
    for base in (0, BASE):
        fs = torch.full((n,), -1, dtype=torch.int64, device=dev)
        keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        ctx.uniq_resolve_device(d_h, n, base, fs, keep)
        assert _status(ctx) == (0, 0)
        got = fs.cpu().numpy()
        assert np.array_equal(got, exp + base), (shard, base, int((got != exp + base).sum()))
        assert np.array_equal(keep.cpu().numpy(), exp_keep), (shard, base)


# ---- 4. one key, a million records ---------------------------------------------------------------------------------------
def _contended(keys, n):
    rng = np.random.default_rng(404)
    if keys == "empty":
        return np.full(n, EMPTY, dtype=np.uint64)
    k = K.clustered(rng, 2)                                         # (two keys: the same first slot)
    return np.full(n, k[0], dtype=np.uint64) if keys == "one" else np.tile(k, n // 2)


@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("keys", ["one", "two", "empty"])
def test_one_key_a_million_records_through_insert_pairs(ctx, keys, order):
    """2^20 records of one key (two alternating; the ~0 key) with their indices descending -- every record beats whatever the
    plain 16-byte peek ahead of the atomic min can have shown, the worst order for trusting it -- and shuffled."""
    n = 1 << 20
    h = _contended(keys, n)
    idx = np.arange(n, dtype=np.uint64)[::-1] + np.uint64(BASE)
    if order == "shuffled":
        idx = np.random.default_rng(405).permutation(idx)
    exp = K.expected_first_seen(h, idx)
    ctx.uniq_reset(2)
    _insert(ctx, "pairs", h, idx)
    got = _lookup(ctx, "pairs", h)
    assert _status(ctx) == (0, 0)
    assert np.array_equal(got, exp), (np.unique(got)[:4], np.unique(exp))


@pytest.mark.parametrize("n", [1 << 20, 1 << 18], ids=["2^20_bucket_fallback", "2^18_direct_table"])
@pytest.mark.parametrize("keys", ["one", "empty"])
def test_one_key_a_million_records_through_resolve(ctx, keys, n):
    """all records equal: 2^20 of them overfill one LDS bucket (the HBM fallback), 2^18 take the table directly -- the split
    low / high value of uniq_fold_local under contention.  Every answer is the first record."""
    import torch
    h = _contended(keys, n)
    exp = K.expected_first_seen(h)
    dev = torch.device("cuda", 0)
    d_h = _dev(h)
    for base in (0, BASE):
        fs = torch.full((n,), -1, dtype=torch.int64, device=dev)
        keep = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        ctx.uniq_resolve_device(d_h, n, base, fs, keep)
        assert _status(ctx) == (0, 0)
        assert np.array_equal(fs.cpu().numpy(), exp + base)
        assert np.array_equal(keep.cpu().numpy(), (exp == np.arange(n)).astype(np.uint8))


# ---- 5. streaming growth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["fresh_ctx", "from_a_reset_table"])
def test_streaming_growth(stream):
    """circkit_uniq_first_seen grows its table when (count + n) * 2 > slots, to the first power of two >= max(65536,
    4 * (count + n)), and carries every entry -- the ~0 key's own slot included -- into the new one.
    fresh_ctx: batches of 32768, 1, 32767, 65536, 300000 records; the first three add up to 65536 records, exactly half of
    the 131072 slots the first batch creates (equality: no growth), the fourth and fifth each force a growth.
    from_a_reset_table: behind uniq_reset(10) (1024 slots) batches of 16 (no growth), 1000 (to 65536 slots), 31752 (32768
    records: (count + n) * 2 == 65536, no growth), 1 (one past it: growth to 262144), 32767, 65536 (131072 records: equality
    again), 300000 (growth to 2^21): three growths, each with the ~0 key to carry, and both sides of the condition.
    The ~0 key is in the first batch and in every later one of more than one record, so after every growth; a tenth of every
    batch repeats keys of earlier batches; the batch of 65536 carries a base_index below all earlier ones, so its indices
    win -- for itself and for the batch after it.  Expected: the restatement over the stream so far with the global indices
    as given, batch by batch, and a lookup of every record of the stream at the end (what a rehash lost shows there)."""
    import torch
    import circkit_amd
    rng = np.random.default_rng(505)
    sizes = [32768, 1, 32767, 65536, 300000]
    if stream == "from_a_reset_table":
        sizes = [16, 1000, 31752] + sizes[1:]
    fresh = K.random_keys(rng, sum(sizes))
    c = circkit_amd.Context(0)
    try:
        if stream == "from_a_reset_table":
            c.uniq_reset(10)
        all_h, all_idx = np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint64)
        used, next_base = 0, 5_000_000_000
        for b, n in enumerate(sizes):
            n_rep = n // 10 if b else 0
            h = np.concatenate([fresh[used:used + n - n_rep], all_h[rng.integers(0, max(len(all_h), 1), size=n_rep)]])
            used += n - n_rep
            if n > 1:
                h[0] = EMPTY
            h = rng.permutation(h)
            base = 1000 if n == 65536 else next_base                # the late batch below all earlier ones
            if n != 65536:
                next_base += n
            all_h = np.concatenate([all_h, h])
            all_idx = np.concatenate([all_idx, np.arange(n, dtype=np.uint64) + np.uint64(base)])
            got = c.uniq_first_seen(h, base)
            exp = K.expected_first_seen(all_h, all_idx)[-n:]
            assert np.array_equal(got, exp), (stream, b, n, int((got != exp).sum()))
        assert _status(c) == (0, 0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        got = _lookup(c, "device", all_h)
        exp = K.expected_first_seen(all_h, all_idx)
        assert np.array_equal(got, exp), (stream, int((got != exp).sum()))
        assert int((exp < 5_000_000_000).sum()) > 65536            # the late batch won records of other batches too
    finally:
        c.close()


# ---- 6. partition, insert_rows / lookup_rows, gather at the edges ------------------------------------------------------------
SENT64, SENT32, PAD = 0x5E5E5E5E5E5E5E5E, 0x5E5E5E5E, 8


def _exchange(ctx, h, base, world):
    """test_uniq_exchange_kernels' assertions (counts; every record its own row; owners in rank order; row contents; through
    insert_rows / lookup_rows / gather to first-seen) for one shard, with sentinels around d_rows, d_slot and d_counts"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(h)
    rows_buf = torch.full(((n + 2 * PAD) * 2,), SENT64, dtype=torch.int64, device=dev)
    slot_buf = torch.full((n + 2 * PAD,), SENT32, dtype=torch.int32, device=dev)
    counts_buf = torch.full((world + PAD,), SENT64, dtype=torch.int64, device=dev)
    rows, slot, counts = rows_buf[2 * PAD:2 * PAD + 2 * n], slot_buf[PAD:PAD + n], counts_buf[:world]
    assert rows_buf.data_ptr() % 16 == 0
    d_h = _dev(h)
    ctx.uniq_partition_device(d_h, n, base, world, rows if n else None, counts, slot if n else None)
    torch.cuda.synchronize()
    owner = K.owner(h, world).astype(np.int64)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(owner, minlength=world)), (n, world)
    assert np.all(counts_buf[world:].cpu().numpy() == SENT64)
    rb, sb = rows_buf.cpu().numpy(), slot_buf.cpu().numpy()
    assert np.all(rb[:2 * PAD] == SENT64) and np.all(rb[2 * PAD + 2 * n:] == SENT64), (n, world)     # untouched outside [0, n)
    assert np.all(sb[:PAD] == SENT32) and np.all(sb[PAD + n:] == SENT32), (n, world)
    r = rb[2 * PAD:2 * PAD + 2 * n].reshape(n, 2).view(np.uint64)
    sl = sb[PAD:PAD + n].astype(np.int64)
    assert len(np.unique(sl)) == n and (n == 0 or (sl.min() >= 0 and sl.max() < n))                 # every record its own row
    assert np.array_equal(r[sl, 0], h) and np.array_equal(r[sl, 1], np.uint64(base) + np.arange(n, dtype=np.uint64))
    assert np.all(np.diff(K.owner(r[:, 0], world).astype(np.int64)) >= 0)                            # owners in rank order
    ctx.uniq_reset(max(n, 1))
    ctx.uniq_insert_rows_device(rows if n else None, n)
    answers = torch.full((n + PAD,), SENT64, dtype=torch.int64, device=dev)
    ctx.uniq_lookup_rows_device(rows if n else None, n, answers)
    exp = K.expected_first_seen(h)
    for want_keep in (True, False):                                                                  # d_keep is nullable
        fs = torch.full((n + PAD,), SENT64, dtype=torch.int64, device=dev)
        keep = torch.full((n + PAD,), 7, dtype=torch.uint8, device=dev)
        ctx.uniq_gather_device(answers, slot if n else None, n, base, fs, keep if want_keep else None)
        assert _status(ctx) == (0, 0)
        fs, keep = fs.cpu().numpy(), keep.cpu().numpy()
        assert np.array_equal(fs[:n], exp + base), (n, world)
        assert np.all(fs[n:] == SENT64) and np.all(keep[n:] == 7)
        assert np.array_equal(keep[:n], (exp == np.arange(n)).astype(np.uint8) if want_keep else np.full(n, 7, dtype=np.uint8))
    assert np.all(answers[n:].cpu().numpy() == SENT64)


@pytest.mark.parametrize("world", [1, 2, 63, 64])
def test_exchange_steps_at_the_chunk_edges(ctx, world):
    """the scatter kernel works in chunks of 1024 keys, four per thread: n = 0 and 1, one row of threads more or less (255,
    256), one chunk more or less (1023, 1024, 1025), five chunks with a tail (4097); worlds 1, 2 and the two next to the
    64-lane prefix sum's width.  Keys repeat about three times, the ~0 key among them."""
    rng = np.random.default_rng(600 + world)
    for n in (0, 1, 255, 256, 1023, 1024, 1025, 4097):
        pool = K.random_keys(rng, max(n // 3, 1))
        h = pool[rng.integers(0, len(pool), size=n)]
        if n >= 2:
            h[rng.integers(0, n, size=2)] = EMPTY
        _exchange(ctx, h, BASE, world)


@pytest.mark.parametrize("world", [2, 63, 64])
@pytest.mark.parametrize("end", ["first_owner", "last_owner"])
def test_exchange_steps_with_every_key_at_one_owner(ctx, world, end):
    """5000 records whose keys all belong to owner 0, or all to owner world - 1: every other owner's count is zero (the
    `hist ? atomicAdd : 0` reservation) and one owner's rows are the whole shard"""
    rng = np.random.default_rng(700 + world)
    pool = K.owned_by(rng, 1700, 0 if end == "first_owner" else world - 1, world)
    _exchange(ctx, pool[rng.integers(0, len(pool), size=5000)], BASE, world)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------
def _refused(fn, *words):
    import circkit_amd
    with pytest.raises(circkit_amd.CirckitError) as e:
        fn()
    assert e.value.code == INVALID_ARG, str(e.value)
    for w in words:
        assert w in str(e.value)


def _answers_a_small_batch(ctx):
    h = np.array([5, 6, 5, EMPTY, 6, EMPTY], dtype=np.uint64)
    ctx.uniq_reset(len(h))
    ctx.uniq_insert_device(_dev(h), len(h), 10)
    assert _lookup(ctx, "device", h).tolist() == [10, 11, 10, 13, 11, 13]
    assert _status(ctx) == (0, 0)


def test_too_many_records_a_bad_world_and_misaligned_rows_are_refused(ctx):
    """n = 2^32 - 1 (the local index 0xFFFFFFFF means "nothing yet"), world 0 and 65, and a d_rows that is not 16-byte aligned
    are refused before anything is launched: the tiny buffers behind the calls keep their sentinels, and the ctx answers a
    small batch after each refusal."""
    import torch
    dev = torch.device("cuda", 0)
    small = lambda dtype=torch.int64: torch.full((8,), SENT32, dtype=dtype, device=dev)      # noqa: E731
    d_h, fs, rows, counts, answers = small(), small(), small(), torch.full((80,), SENT32, dtype=torch.int64, device=dev), small()
    slot, keep = small(torch.int32), torch.full((8,), 7, dtype=torch.uint8, device=dev)
    too_many = (1 << 32) - 1

    def untouched():
        torch.cuda.synchronize()
        for t in (d_h, fs, rows, counts, answers, slot):
            assert bool((t == SENT32).all())
        assert bool((keep == 7).all())

    refusals = [
        (lambda: ctx.uniq_resolve_device(d_h, too_many, 0, fs, keep), ("2^32",)),
        (lambda: ctx.uniq_partition_device(d_h, too_many, 0, 2, rows, counts, slot), ("2^32",)),
        (lambda: ctx.uniq_partition_device(d_h, 4, 0, 0, rows, counts, slot), ()),
        (lambda: ctx.uniq_partition_device(d_h, 4, 0, 65, rows, counts, slot), ()),
        (lambda: ctx.uniq_partition_device(d_h, 3, 0, 2, rows[1:], counts, slot), ("16-byte",)),
        (lambda: ctx.uniq_insert_rows_device(rows[1:], 3), ("16-byte",)),
        (lambda: ctx.uniq_lookup_rows_device(rows[1:], 3, answers), ("16-byte",)),
    ]
    assert rows.data_ptr() % 16 == 0 and rows[1:].data_ptr() % 16 == 8
    for with_table in (False, True):                                # on a ctx without a table, and on one with
        for fn, words in refusals:
            _refused(fn, *words)
            untouched()
            if with_table:
                _answers_a_small_batch(ctx)
        _answers_a_small_batch(ctx)


TABLE_CALLS = {
    "insert": lambda c, t: c.uniq_insert_device(t["h"], 4, 0),
    "insert_pairs": lambda c, t: c.uniq_insert_pairs_device(t["h"], t["h"], 4),
    "lookup": lambda c, t: c.uniq_lookup_device(t["h"], 4, t["out"]),
    "insert_rows": lambda c, t: c.uniq_insert_rows_device(t["h"], 2),
    "lookup_rows": lambda c, t: c.uniq_lookup_rows_device(t["h"], 2, t["out"]),
}


def _table_call_buffers():
    import torch
    dev = torch.device("cuda", 0)
    return {"h": torch.arange(1, 5, dtype=torch.int64, device=dev), "out": torch.full((4,), SENT64, dtype=torch.int64, device=dev)}


@pytest.mark.parametrize("call", sorted(TABLE_CALLS))
def test_table_calls_before_any_reset_are_refused(ctx, call):
    import torch
    t = _table_call_buffers()
    _refused(lambda: TABLE_CALLS[call](ctx, t), "circkit_uniq_reset has not been called")
    torch.cuda.synchronize()
    assert bool((t["out"] == SENT64).all())
    _answers_a_small_batch(ctx)


def test_table_calls_after_a_resolve_are_refused(ctx):
    """a resolve leaves the table in a layout of its own (or none at all): the table calls refuse until the next reset"""
    import torch
    t = _table_call_buffers()
    fs = torch.empty(4, dtype=torch.int64, device=t["h"].device)
    for call in sorted(TABLE_CALLS):
        ctx.uniq_resolve_device(t["h"], 4, BASE, fs, None)
        assert fs.tolist() == [BASE, BASE + 1, BASE + 2, BASE + 3]
        _refused(lambda: TABLE_CALLS[call](ctx, t), "circkit_uniq_reset has not been called")
        torch.cuda.synchronize()
        assert bool((t["out"] == SENT64).all())
        _answers_a_small_batch(ctx)


# ---- 8. the table's state: one per ctx, and none of it borrowed ------------------------------------------------------------
def test_table_state_is_per_ctx():
    """Two ctxs on device 0, their calls interleaved one by one: the same 3000 keys go into both tables, with base_index 0 in A
    and 1 000 000 in B, and each answers with its own indices.  Then A alone overflows (uniq_reset(1): 1024 slots, 3000 distinct
    keys): A's status counts the 1976 keys that found no slot, B's stays clean and B's answers stay what they were -- the
    table, its overflow counter and the rest of the uniq state belong to one ctx each.  B still answers after A is destroyed."""
    import torch
    import circkit_amd
    n, base_b = 3000, 1_000_000
    h = K.random_keys(np.random.default_rng(808), n)
    i = np.arange(n, dtype=np.uint64)
    a, b = circkit_amd.Context(0), circkit_amd.Context(0)
    try:
        for c in (a, b):
            c.set_stream(torch.cuda.current_stream().cuda_stream)
        d_h = _dev(h)
        a.uniq_reset(4096)
        b.uniq_reset(4096)
        a.uniq_insert_device(d_h, n, 0)
        b.uniq_insert_device(d_h, n, base_b)
        got_a, got_b = _lookup(a, "device", h), _lookup(b, "device", h)
        assert np.array_equal(got_a, i)
        assert np.array_equal(got_b, i + np.uint64(base_b))
        assert _status(a) == (0, 0) and _status(b) == (0, 0)

        a.uniq_reset(1)
        a.uniq_insert_device(d_h, n, 0)
        answered = _lookup(a, "device", h) != EMPTY
        assert int(answered.sum()) == 1024
        assert _status(a) == (OOM, int((~answered).sum())) and int((~answered).sum()) == n - 1024
        assert _status(b) == (0, 0)
        assert np.array_equal(_lookup(b, "device", h), i + np.uint64(base_b))

        a.close()
        assert np.array_equal(_lookup(b, "device", h), i + np.uint64(base_b))
        assert _status(b) == (0, 0)
    finally:
        a.close()
        b.close()


def test_the_host_form_owns_its_staging():
    """circkit_uniq_first_seen between two host canonicalize batches on one ctx, with more keys (5000) than anything the ctx has
    staged (8 records): the batch of 8 records of 64 bases gives the same bytes, hashes, indices and strands before and after --
    those of the oracle -- and both first-seen arrays (5000 keys, half of them repeats; 500 more from base_index 5000, 100 of
    them keys of the first batch) are the restatement over the joined stream."""
    import circkit_amd
    from oracle import oracle
    rng = np.random.default_rng(909)
    data = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=8 * 64)]
    offsets = np.arange(9, dtype=np.uint64) * np.uint64(64)
    exp_bytes, exp_hash = oracle.canonicalize_batch(data, offsets, want_bytes=True, want_hash=True)
    pool = K.random_keys(rng, 2500 + 400)
    h1 = rng.permutation(np.concatenate([pool[:2500], pool[:2500]]))
    h2 = rng.permutation(np.concatenate([h1[rng.choice(5000, size=100, replace=False)], pool[2500:]]))
    exp = K.expected_first_seen(np.concatenate([h1, h2]))
    c = circkit_amd.Context(0)
    try:
        canon = lambda: c.canonicalize_batch(data, offsets, want_bytes=True, want_index=True, want_strand=True, want_xxh3=True)   # noqa: E731
        first = canon()
        fs1 = c.uniq_first_seen(h1, 0)
        second = canon()
        fs2 = c.uniq_first_seen(h2, 5000)
        for out in (first, second):
            assert np.array_equal(out["bytes"], exp_bytes)
            assert np.array_equal(out["xxh3"], exp_hash)
        assert np.array_equal(first["index"], second["index"]) and np.array_equal(first["strand"], second["strand"])
        assert np.array_equal(fs1, exp[:5000].astype(np.uint64)), int((fs1 != exp[:5000]).sum())
        assert np.array_equal(fs2, exp[5000:].astype(np.uint64)), int((fs2 != exp[5000:]).sum())
        assert _status(c) == (0, 0)
    finally:
        c.close()
