"""Seeded key generators (NumPy only) that aim the uniq table's tests at the code random keys never reach, and the plain
restatement of first-seen every such test compares against.

The generators mirror two functions of circkit_amd/csrc/circkit_uniq.hip -- only to AIM the input:
  uniq_slot(h, mask) = (h ^ (h >> 29)) & mask        where a key starts probing (clustered)
  bkt_of(h, log2b)   = h >> (64 - log2b)             which LDS bucket a key of a bucketed resolve goes to (top_bits, bucket_shard)
and one that is a contract written in include/circkit.h:
  owner(h, world)    = ((h >> 20) & 0x7FFFFFFF) % world   (owned_by)
Expected values never depend on any of them: they come from expected_first_seen alone.  If uniq_slot or bkt_of changes, these
generators must follow, or the tests that use them lose their aim silently (they would still pass, on keys that spread evenly);
tests/test_uniq_keys_cpu.py checks the generators against the formulas as written HERE, not against the kernels."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)      # the table's EMPTY marker: as a key it has a slot of its own
BKT_MAX = 3072                             # rows of one bucket that are still resolved in LDS (one more: the HBM fallback)
BKT_KEYS = 2600                            # the sizing rule: the smallest 2^log2b >= 64 buckets with BKT_KEYS << log2b >= n
_M24 = np.uint64(0xFFFFFF)


def mix(h):
    """the table's slot function before the mask"""
    h = np.asarray(h, dtype=np.uint64)
    return h ^ (h >> np.uint64(29))


def owner(h, world):
    h = np.asarray(h, dtype=np.uint64)
    return ((h >> np.uint64(20)) & np.uint64(0x7FFFFFFF)) % np.uint64(world)


def bucket_log2(n):
    """buckets (log2) of a bucketed resolve of n keys"""
    log2b = 6
    while log2b < 13 and (BKT_KEYS << log2b) < n:
        log2b += 1
    return log2b


def bkt_of(h, log2b):
    """the bucket of a key in a bucketed resolve of 2^log2b buckets: its top log2b bits"""
    return (np.asarray(h, dtype=np.uint64) >> np.uint64(64 - log2b)).astype(np.int64)


def _distinct(rng, n, draw):
    """n distinct values of draw(k) (k values per call), in a seeded random order"""
    got = np.empty(0, dtype=np.uint64)
    while len(got) < n:
        got = np.unique(np.concatenate([got, draw(2 * (n - len(got)) + 16)]))
    return rng.permutation(got)[:n]


def random_keys(rng, n):
    """n distinct uniformly random keys, none equal to ~0 (what every earlier test of the table feeds it)"""
    def draw(k):
        h = rng.integers(0, 1 << 64, size=k, dtype=np.uint64)
        return h[h != EMPTY]
    return _distinct(rng, n, draw)


def clustered(rng, n, tail=3, top_bits=None):
    """n distinct 64-bit keys, none equal to ~0, whose mixed low 24 bits, (h ^ (h >> 29)) & 0xFFFFFF, are 0xFFFFFF - tail + 1:
    in every power-of-two table of up to 2^24 slots -- the 4096-slot LDS table of the bucketed resolve included -- all of them
    start probing `tail` slots before the end, so more than `tail` of them make one cluster that wraps to slot 0.
    top_bits = (value, nbits) fixes the top nbits (<= 32) bits, which select the bucket of a bucketed resolve.

    Bits 24..63 are chosen freely; (h >> 29) & 0xFFFFFF reads bits 29..52 only, so the low 24 bits follow as
    target ^ ((h >> 29) & 0xFFFFFF).  (~0 mixes to 0 in its low 24 bits: no tail gives it.)

    This mirrors uniq_slot only to aim the input; see the module docstring."""
    assert 1 <= tail < (1 << 24)
    target = np.uint64(0xFFFFFF - tail + 1)
    value, nbits = top_bits if top_bits else (0, 0)
    assert 0 <= nbits <= 32 and 0 <= value < (1 << nbits)
    free = 40 - nbits
    hi = _distinct(rng, n, lambda k: rng.integers(0, 1 << free, size=k, dtype=np.uint64))
    h = ((np.uint64(value) << np.uint64(free)) | hi) << np.uint64(24)
    return h | (target ^ ((h >> np.uint64(29)) & _M24))


def owned_by(rng, n, owner_rank, world):
    """n distinct keys, none equal to ~0, with ((h >> 20) & 0x7FFFFFFF) % world == owner_rank (the contract of include/circkit.h)"""
    assert 0 <= owner_rank < world
    qmax = (0x7FFFFFFF - owner_rank) // world

    def draw(k):
        mid = rng.integers(0, qmax + 1, size=k, dtype=np.uint64) * np.uint64(world) + np.uint64(owner_rank)
        low = rng.integers(0, 1 << 20, size=k, dtype=np.uint64)
        top = rng.integers(0, 1 << 13, size=k, dtype=np.uint64)
        h = (top << np.uint64(51)) | (mid << np.uint64(20)) | low
        return h[h != EMPTY]
    return _distinct(rng, n, draw)


def bucket_shard(rng, n, bucket, rows, empty_rows=0):
    """A shard of n keys for a bucketed resolve of 2^log2b buckets (bucket_log2(n)) in which bucket `bucket` holds exactly
    `rows` rows: rows - empty_rows distinct clustered keys with that bucket's top bits (one probe chain in the 4096-slot LDS
    table, wrapping at slot 4095) and empty_rows copies of the ~0 key (bucket 2^log2b - 1 only).  The other n - rows records are
    random keys of the other buckets, each about three times, far below BKT_MAX rows per bucket.  Records in random order."""
    log2b = bucket_log2(n)
    B = 1 << log2b
    assert 0 <= bucket < B and (empty_rows == 0 or bucket == B - 1) and empty_rows <= rows <= n
    chain = clustered(rng, rows - empty_rows, top_bits=(bucket, log2b))
    rest_n = n - rows
    pool = rng.integers(0, 1 << (64 - log2b), size=max(rest_n // 3, 1), dtype=np.uint64)
    other = rng.integers(0, B - 1, size=len(pool), dtype=np.uint64)
    other += (other >= np.uint64(bucket)).astype(np.uint64)                    # any bucket but the chosen one
    pool |= other << np.uint64(64 - log2b)
    rest = pool[rng.integers(0, len(pool), size=rest_n)]
    h = np.concatenate([chain, np.full(empty_rows, EMPTY, dtype=np.uint64), rest])
    return rng.permutation(h)


def expected_first_seen(h, index=None):
    """The plain restatement: for every record the smallest index among the records with its key.  index: the records' global
    indices (any integer dtype, returned in it); None = 0 .. n - 1 (int64)"""
    h = np.asarray(h)
    if index is None:
        index = np.arange(len(h), dtype=np.int64)
        order = np.argsort(h, kind="stable")                    # stable: the first of each run is the smallest index
    else:
        index = np.asarray(index)
        order = np.lexsort((index, h))                          # by key, then by index
    hs = h[order]
    first_of_group = np.r_[True, hs[1:] != hs[:-1]] if len(h) else np.zeros(0, dtype=bool)
    group_first_idx = index[order][first_of_group]
    group_id = np.cumsum(first_of_group) - 1
    fs = np.empty(len(h), dtype=index.dtype)
    fs[order] = group_first_idx[group_id]
    return fs
