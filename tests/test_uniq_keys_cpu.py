"""The key generators of tests/uniq_keys.py give what they claim (no GPU): tests/test_uniq_table_gpu.py is only as sharp as
its inputs, and a generator that quietly stopped clustering would leave those tests passing on harmless keys."""
import numpy as np
import pytest

from tests import uniq_keys as K


@pytest.mark.parametrize("tail", [1, 3, 700])
@pytest.mark.parametrize("top_bits", [None, (0xAB, 8), (255, 8), (0, 8), (5, 6), (8191, 13)])
def test_clustered_keys_start_tail_slots_before_the_end_of_every_table(tail, top_bits):
    rng = np.random.default_rng(1)
    n = 3073
    h = K.clustered(rng, n, tail=tail, top_bits=top_bits)
    assert h.dtype == np.uint64 and len(h) == n
    assert len(np.unique(h)) == n                                   # distinct
    assert not np.any(h == K.EMPTY)                                 # never the EMPTY marker
    for log2 in range(10, 25):                                      # masks 2^10 - 1 .. 2^24 - 1 (4096: the LDS table's)
        slots = 1 << log2
        start = K.mix(h) & np.uint64(slots - 1)
        assert np.all(start == np.uint64((slots - tail) % slots)), (log2, tail)
    if top_bits:
        value, nbits = top_bits
        assert np.all(h >> np.uint64(64 - nbits) == np.uint64(value))
    # seeded: the same rng state gives the same keys
    assert np.array_equal(h, K.clustered(np.random.default_rng(1), n, tail=tail, top_bits=top_bits))


@pytest.mark.parametrize("world", [1, 2, 3, 63, 64])
def test_owned_by_puts_every_key_at_its_owner(world):
    rng = np.random.default_rng(2)
    for owner in sorted({0, world // 2, world - 1}):
        h = K.owned_by(rng, 5000, owner, world)
        assert h.dtype == np.uint64 and len(np.unique(h)) == 5000 and not np.any(h == K.EMPTY)
        assert np.all(K.owner(h, world) == owner)
        # the formula of include/circkit.h, written out once more on Python integers
        assert all(((int(x) >> 20) & 0x7FFFFFFF) % world == owner for x in h[:200])
        assert len(np.unique(h >> np.uint64(51))) > 1000 and len(np.unique(h & np.uint64(0xFFFFF))) > 1000     # the other bits vary


@pytest.mark.parametrize("bucket,rows,empty_rows", [(0xAB, 3072, 0), (0xAB, 3073, 0), (255, 3072, 500)])
def test_bucket_shards_hold_exactly_the_rows_they_claim(bucket, rows, empty_rows):
    """the three shards of test_uniq_table_gpu.py's bucket-boundary test, generated the same way"""
    n = 1 << 19
    assert K.bucket_log2(n) == 8 and K.bucket_log2(n + 1) == 8 and K.bucket_log2((2600 << 8) + 1) == 9 and K.bucket_log2(1000) == 6
    h = K.bucket_shard(np.random.default_rng(3), n, bucket, rows, empty_rows)
    assert h.dtype == np.uint64 and len(h) == n
    counts = np.bincount((h >> np.uint64(56)).astype(np.int64), minlength=256)        # rows per bucket, from the top 8 bits
    assert counts[bucket] == rows
    others = np.delete(counts, bucket)
    assert others.max() < K.BKT_MAX and others.min() > 0            # only the chosen bucket is at the boundary
    assert int((h == K.EMPTY).sum()) == empty_rows
    chain = h[(h >> np.uint64(56) == np.uint64(bucket)) & (h != K.EMPTY)]
    assert len(np.unique(chain)) == rows - empty_rows               # distinct keys,
    assert np.all(K.mix(chain) & np.uint64(4095) == np.uint64(4093))        # one chain that starts 3 slots before the LDS table's end
    assert len(np.unique(h)) < n // 2                               # the rest repeats (about 3x)
    # the bucket's rows are spread over the shard, not one block of it
    where = np.flatnonzero(h >> np.uint64(56) == np.uint64(bucket))
    assert where.min() < n // 8 and where.max() > n - n // 8


def test_expected_first_seen_against_the_oracle():
    from oracle import oracle as O
    rng = np.random.default_rng(4)
    for n, distinct in ((0, 1), (1, 1), (2, 1), (1000, 10), (1000, 1000), (50_000, 7000)):
        h = rng.integers(0, distinct, size=n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        if n > 2:
            h[rng.integers(0, n, 3)] = K.EMPTY
        fs = K.expected_first_seen(h)
        assert fs.dtype == np.int64
        assert np.array_equal(fs.astype(np.uint64), O.uniq_first_seen(h)), n
        # explicit indices: any permutation of the records with their indices gives each record the same answer
        p = rng.permutation(n)
        idx = np.arange(n, dtype=np.uint64) + np.uint64(7_000_000_000)
        fs_p = K.expected_first_seen(h[p], idx[p])
        assert fs_p.dtype == np.uint64
        assert np.array_equal(fs_p, (fs[p] + 7_000_000_000).astype(np.uint64)), n


def test_expected_first_seen_takes_the_smallest_index_not_the_first_position():
    h = np.array([7, 7, 9, 7, 9], dtype=np.uint64)
    idx = np.array([50, 40, 30, 45, 31], dtype=np.uint64)
    assert K.expected_first_seen(h, idx).tolist() == [40, 40, 30, 40, 30]
    assert K.expected_first_seen(h).tolist() == [0, 0, 2, 0, 2]
