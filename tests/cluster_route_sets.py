"""Input sets that aim a candidates call at every route of circkit_uniq_resolve_device (TEST INFRASTRUCTURE ONLY).  The resolve
chooses by the number of keys, n_records * n_bands: below CK_UNIQ_BUCKET_MIN the HBM table directly; up to BKT_KEYS << BKT_MAX_LOG2
keys LDS buckets, and the HBM table behind them when a bucket holds more than BKT_MAX rows; beyond that the table again.  Every set
is seeded and the smallest that reaches its route; tests/test_cluster_route_sets_cpu.py establishes the route of each from the
yardstick's keys (tests/cluster_np.py) and tests/uniq_keys.py's bucket function, and holds the constants below against the source.
Expected values come from tests/cluster_np.py alone."""
import functools
import os
import re

import numpy as np

from tests import cluster_np as N
from tests import uniq_keys as K

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
BUCKET_MIN = 1 << 19                    # CK_UNIQ_BUCKET_MIN
BKT_MAX_LOG2 = 13
BUCKET_LIMIT = K.BKT_KEYS << BKT_MAX_LOG2       # the last number of keys that is resolved in buckets
EMPTY = N.EMPTY

# name: (records, bands, band_bins, bins of a row, seed)
SETS = {
    "direct_last": (8191, 64, 1, 64, 4101),
    "lds_first": (8192, 64, 1, 64, 4102),
    "lds_63": (8323, 63, 1, 64, 4103),
    "lds_5x3": (104_858, 5, 3, 16, 4104),
    "no_key_flood": (8192, 64, 1, 64, 4105),
    "identical": (8192, 64, 1, 64, 4106),
    "beyond_buckets": (332_801, 64, 1, 64, 4107),
}
LDS = ("lds_first", "lds_63", "lds_5x3")        # resolved in LDS: no bucket above BKT_MAX rows
FALLBACK = ("no_key_flood", "identical")        # bucketed, a bucket above BKT_MAX rows: the HBM table behind the buckets
FLOOD_EMPTY = 0.05


def source_constants():
    """BKT_MAX, BKT_KEYS, BKT_MAX_LOG2 and CK_UNIQ_BUCKET_MIN as circkit_uniq.hip has them: the three from the one constexpr line
    that declares them, the threshold from its preprocessor macro."""
    from tests.grid_sets import _value
    src = open(os.path.join(CSRC, "circkit_uniq.hip")).read()
    line = [ln for ln in src.splitlines() if ln.lstrip().startswith("constexpr") and "BKT_MAX_LOG2" in ln]
    assert len(line) == 1 and "BKT_MAX " in line[0] and "BKT_KEYS" in line[0], line
    c = {name: _value(line[0], name) for name in ("BKT_MAX", "BKT_KEYS", "BKT_MAX_LOG2")}
    m = re.findall(r"^#define CK_UNIQ_BUCKET_MIN \((\d+)u << (\d+)\)", src, flags=re.M)
    assert len(m) == 1, m
    c["CK_UNIQ_BUCKET_MIN"] = int(m[0][0]) << int(m[0][1])
    return c


def planted_rows(rng, n, n_bands, band_bins, bins):
    """Random rows without an EMPTY bin in which about every second record holds two to four single bands of one or two earlier
    records: the first copy goes to band 0, the last band or the middle one in turn, the second to another of the three, the
    others anywhere.  A copy takes the source's band as drawn, so a key is held by few records.  The last record always copies:
    band 0 and the last band, from two records that copy nothing themselves."""
    base = rng.integers(0, 2 ** 63, size=(n, bins), dtype=np.uint64)
    rows = base.copy()
    i = np.arange(n)
    plant = rng.random(n) < 0.5
    plant[0] = False
    n_copies = rng.integers(2, 5, size=n)
    src_a = (rng.random(n) * i).astype(np.int64)                     # an earlier record (record 0 copies nothing)
    src_b = np.where(rng.random(n) < 0.5, (rng.random(n) * i).astype(np.int64), src_a)
    aimed = np.array([0, n_bands - 1, n_bands // 2])
    bin_of = np.arange(band_bins)
    for c in range(4):
        band = aimed[(i + c) % 3] if c < 2 else rng.integers(0, n_bands, size=n)
        src = src_a if c % 2 == 0 else src_b
        at = np.flatnonzero(plant & (c < n_copies))
        at = at[at != n - 1]
        cols = band[at, None] * band_bins + bin_of[None, :]
        rows[at[:, None], cols] = base[src[at, None], cols]
    plain = np.flatnonzero(~plant[:n - 1])
    a, b = (int(v) for v in rng.choice(plain, size=2, replace=False))
    rows[n - 1, 0:band_bins] = base[a, 0:band_bins]
    rows[n - 1, (n_bands - 1) * band_bins:n_bands * band_bins] = base[b, (n_bands - 1) * band_bins:n_bands * band_bins]
    return rows


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """(rows, n_bands, band_bins) of a set; the rows are read-only."""
    n, nb, bb, bins, seed = SETS[name]
    rng = np.random.default_rng(seed)
    if name == "identical":
        rows = np.repeat(rng.integers(0, 2 ** 63, size=(1, bins), dtype=np.uint64), n, axis=0)
    else:
        rows = planted_rows(rng, n, nb, bb, bins)
    if name == "no_key_flood":
        rows[rng.random(rows.shape) < FLOOD_EMPTY] = EMPTY
        # the last record proposes all the same: its first and its last bin are two earlier records' that kept theirs
        for col in (0, nb * bb - 1):
            held = np.flatnonzero(rows[:n - 1, col] != EMPTY)
            rows[n - 1, col] = rows[int(rng.choice(held)), col]
    rows.setflags(write=False)
    return rows, nb, bb


def n_keys(name):
    n, nb = SETS[name][:2]
    return n * nb


@functools.lru_cache(maxsize=None)
def keys_of(name):
    rows, nb, bb = rows_of(name)
    keys = N.band_keys(rows, nb, bb)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def expected(name):
    """(offsets, pairs) of the yardstick, computed once and kept (read-only)."""
    rows, nb, bb = rows_of(name)
    offsets, pairs = N.candidates(rows, nb, bb, keys=keys_of(name))
    offsets.setflags(write=False)
    pairs.setflags(write=False)
    return offsets, pairs


def max_bucket(name):
    """The rows of the fullest bucket of the bucketed resolve of the set's keys."""
    keys = keys_of(name).reshape(-1)
    return int(np.bincount(K.bkt_of(keys, K.bucket_log2(len(keys)))).max())
