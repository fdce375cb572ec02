"""Input sets of the cluster unit, shared by its CPU fiber test and its GPU test (TEST INFRASTRUCTURE ONLY).  Everything is seeded,
and the yardstick's answer for a set is computed once and kept."""
import functools
import os
import re

import numpy as np

from tests import cluster_ref as C
from tests import sketch_ref as R
from tests import sketch_sets as SS

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
EMPTY = np.uint64(R.EMPTY)
PASS = (10, 10)                         # a (match, filled) that every threshold of the sets lets through
DEFAULT = (C.q16(0.2), 8)


def constants():
    """The launch constants of circkit_cluster.hip and the scan's of cluster.h, read from the sources."""
    from tests.grid_sets import _value
    src, hdr = open(os.path.join(CSRC, "circkit_cluster.hip")).read(), open(os.path.join(CSRC, "cluster.h")).read()
    c = {name: _value(src, name) for name in ("KEYS_WG", "KEYS_MAX_GRID", "EMIT_WAVES", "EMIT_MAX_GRID", "LINK_WG", "LINK_MAX_GRID", "FLATTEN_MAX_GRID")}
    for name in ("SCAN_WG", "SCAN_ITEMS"):
        c[name] = _value(hdr, name)
    return c


# ---- candidates ----------------------------------------------------------------------------------------------------------------
def random_rows(rng, n, bins):
    return rng.integers(0, 2 ** 63, size=(n, bins), dtype=np.uint64)


def _band(b, band_bins):
    return slice(b * band_bins, (b + 1) * band_bins)


def key_of_none(prefix, b):
    """The last bin of a band whose earlier bins are `prefix`, chosen so that the band's key comes out as 2^64 - 1."""
    x = ((b + 1) * C.GOLDEN) & R.MASK
    for v in prefix:
        x = R.fmix64(x ^ int(v))
    v = R.fmix64_inverse(C.NO_KEY) ^ x
    assert v != R.EMPTY
    return v


def family_rows(rng, n, bins, empty=0.03):
    """Rows of which many hold stretches copied from earlier rows, with EMPTY bins sprinkled in."""
    rows = random_rows(rng, n, bins)
    for i in range(1, n):
        for _ in range(int(rng.integers(0, 4))):
            j = int(rng.integers(0, i))
            a = 0 if rng.random() < 0.3 else int(rng.integers(0, bins))       # (often from the first bin: a 1 x 1 banding reads no other)
            b = min(bins, a + int(rng.integers(min(16, bins // 2), max(17, bins // 2))))
            rows[i, a:b] = rows[j, a:b]
    rows[rng.random(rows.shape) < empty] = EMPTY
    return rows


@functools.lru_cache(maxsize=None)
def candidate_cases():
    """{name: (rows, n_bands, band_bins)}"""
    rng = np.random.default_rng(2101)
    cases = {}
    # the shared band first, in the middle, last and everywhere between: record r shares band r - 1 with record 0 and nothing else
    for nb, bb, bins in ((8, 2, 16), (64, 1, 64), (5, 3, 16)):
        rows = random_rows(rng, nb + 1, bins)
        for r in range(1, nb + 1):
            rows[r, _band(r - 1, bb)] = rows[0, _band(r - 1, bb)]
        cases["shared_%dx%d" % (nb, bb)] = (rows, nb, bb)
    # record 1 equals record 0 in bands 2, 3, 4 of 8; bands 2 and 4 hold one EMPTY bin (their last / their first): band 3 alone
    # proposes.  Record 2 equals record 0 in band 2 only: nothing.  Record 3 equals record 1 in band 4 only: nothing.
    rows = random_rows(rng, 4, 32)
    rows[0, 2 * 4 + 3] = rows[0, 4 * 4] = EMPTY
    rows[1, 8:20] = rows[0, 8:20]
    rows[2, 8:12] = rows[0, 8:12]
    rows[3, 16:20] = rows[1, 16:20]
    cases["empty_beside_equal"] = (rows, 8, 4)
    rows = random_rows(rng, 9, 16)
    rows[[0, 3, 4, 8]] = EMPTY
    rows[6] = rows[2]
    cases["all_empty_rows"] = (rows, 4, 4)
    # a key forced to 2^64 - 1: records 0 and 1 share it in band 1 (one bin) and would pair if it were a key; 2 and 3 in band 2
    # of two bins; record 4 shares a real key with record 0 in band 3
    rows = random_rows(rng, 5, 16)
    rows[0, 1] = rows[1, 1] = key_of_none([], 1)
    rows[4, 3] = rows[0, 3]
    cases["no_key_1bin"] = (rows.copy(), 16, 1)
    rows = random_rows(rng, 5, 16)
    rows[2, 5] = key_of_none([rows[2, 4]], 2)
    rows[3, 4:6] = rows[2, 4:6]
    rows[4, 6:8] = rows[0, 6:8]
    cases["no_key_2bins"] = (rows, 8, 2)
    # record 5: band 0 with 2, band 1 with 0, band 2 with 2 again, band 3 with 4, band 4 with 0 again; records 1 and 3 both hold
    # record 0's band 5 (3 pairs with 0, not with 1); record 6 holds 5's band 7 and 3's band 6
    rows = random_rows(rng, 7, 16)
    rows[5, _band(0, 2)], rows[5, _band(1, 2)], rows[5, _band(2, 2)] = rows[2, _band(0, 2)], rows[0, _band(1, 2)], rows[2, _band(2, 2)]
    rows[5, _band(3, 2)], rows[5, _band(4, 2)] = rows[4, _band(3, 2)], rows[0, _band(4, 2)]
    rows[1, _band(5, 2)] = rows[3, _band(5, 2)] = rows[0, _band(5, 2)]
    rows[6, _band(7, 2)], rows[6, _band(6, 2)] = rows[5, _band(7, 2)], rows[3, _band(6, 2)]
    cases["several_earlier"] = (rows, 8, 2)
    row = random_rows(rng, 1, 64)
    cases["identical_x1000"] = (np.repeat(row, 1000, axis=0), 64, 1)
    for nb, bb, lb in ((1, 1, 10), (64, 1, 10), (1, 16, 10), (64, 16, 10), (16, 1, 4), (1, 16, 4)):
        cases["corner_%dx%d_bins%d" % (nb, bb, 1 << lb)] = (family_rows(rng, 24, 1 << lb, empty=0.002 if bb == 16 else 0.03), nb, bb)
    for n in (0, 1, 63, 64, 65):
        cases["records_%d" % n] = (family_rows(rng, n, 16), 4, 2)
    return cases


@functools.lru_cache(maxsize=None)
def past_the_emit_grid():
    """One record past the count / write kernels' grid, which at 64 bands is also past the keys kernel's: rows drawn from 40
    distinct ones, so that most records find an earlier holder of some band."""
    c = constants()
    n = c["EMIT_MAX_GRID"] * c["EMIT_WAVES"] + 1
    assert n * 64 > c["KEYS_MAX_GRID"] * c["KEYS_WG"]
    rng = np.random.default_rng(2102)
    pool = family_rows(rng, 40, 64)
    return pool[rng.integers(0, 40, size=n)], 64, 1


@functools.lru_cache(maxsize=None)
def expected_candidates(name):
    rows, nb, bb = past_the_emit_grid() if name == "past_the_emit_grid" else candidate_cases()[name]
    offsets, pairs = C.candidates([[int(v) for v in row] for row in rows], nb, bb)
    return np.array(offsets, dtype=np.uint64), np.array(pairs, dtype=np.uint32).reshape(-1, 2)


def pair_buffer(offsets, pairs, capacity, unwritten):
    """What the pair buffer of `capacity` pairs holds: the pairs of every record that ends at or below the capacity."""
    buf = np.full((capacity, 2), unwritten, dtype=np.uint32)
    for i in range(len(offsets) - 1):
        a, b = int(offsets[i]), int(offsets[i + 1])
        if b <= capacity:
            buf[a:b] = pairs[a:b]
    return buf


# ---- link ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def link_cases():
    """{name: (n, pairs, scores, (min_similarity_q16, min_filled))}"""
    q20, q25 = C.q16(0.2), 16384
    cases = {
        "no_pairs": (10, [], [], DEFAULT),
        "all_rejected": (6, [(0, 1), (2, 3), (4, 5), (1, 2)], [(1, 100), (0, 50), (7, 7), (19, 100)], DEFAULT),
        "filled_below_min": (4, [(0, 1), (2, 3)], [(7, 7), (8, 8)], DEFAULT),
        "ratio_one_below": (4, [(0, 1), (2, 3)], [(24, 100), (25, 100)], (q25, 8)),       # 25 << 16 == 16384 * 100 exactly
        "ratio_0.2": (4, [(0, 1), (2, 3)], [(19, 100), (20, 100)], (q20, 8)),
        "zero_zero": (4, [(0, 1), (2, 3)], [(0, 0), (1, 1)], (0, 1)),
        "threshold_0": (6, [(0, 1), (2, 3), (4, 5)], [(0, 8), (0, 7), (0, 1024)], (0, 8)),
        "threshold_65536": (6, [(0, 1), (2, 3), (4, 5)], [(8, 8), (1023, 1024), (1024, 1024)], (65536, 8)),
        "self_pairs": (5, [(1, 1), (0, 0), (3, 4), (4, 4), (2, 2)], [PASS] * 5, DEFAULT),
        "invalid_among_valid": (5, [(0, 1), (5, 0), (1, 2), (0, 5), (2 ** 32 - 1, 2 ** 32 - 1), (5, 5), (3, 4), (4, 2 ** 31)],
                                [PASS] * 8, DEFAULT),
        "duplicates": (6, [(0, 3), (0, 3), (3, 0), (3, 5), (3, 5), (0, 3)], [PASS] * 6, DEFAULT),
        "both_orientations": (8, [(7, 0), (1, 6), (6, 7), (5, 2), (2, 3), (4, 3)], [PASS] * 6, DEFAULT),
        "duplicate_rejected_once": (4, [(0, 1), (0, 1), (2, 3)], [(1, 100), PASS, (1, 100)], DEFAULT),
    }
    return cases


def _shuffled(rng, pairs):
    pairs = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    pairs = pairs[rng.permutation(len(pairs))]
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    return pairs


CONTENTION = ("star", "path", "clique", "two_joined_last", "many_components")


@functools.lru_cache(maxsize=None)
def contention(name, small=False):
    """(n, pairs, scores, params) of a shape that makes many lanes change the same roots at once; small: the scaled-down version
    the fibers run.  Every shape holds rejected pairs that would join what must stay apart."""
    rng = np.random.default_rng(2200 + CONTENTION.index(name))
    if name == "star":
        leaves = 1000 if small else 100_000
        n = leaves + 3
        pairs = [(0, i) for i in range(1, leaves + 1)]
        bad = [(0, leaves + 1), (5, leaves + 2)]
    elif name == "path":
        n = 500 if small else 50_000
        pairs = [(i, i + 1) for i in range(n - 1)]
        bad = []
    elif name == "clique":
        k = 40 if small else 300
        n = k + 2
        pairs = [(i, j) for i in range(1, k + 1) for j in range(i + 1, k + 1)]
        bad = [(0, 1), (k, k + 1)]
    elif name == "two_joined_last":
        size = 300 if small else 20_000
        n = 2 * size
        parts = [[(int(rng.integers(0, i)) + base, i + base) for i in range(1, size)] for base in (0, size)]
        pairs = parts[0] + parts[1]
        bad = []
    elif name == "many_components":
        count, size = (40, 10) if small else (2000, 50)
        n = count * size
        order = rng.permutation(n)                                                  # component c = order[c * size : (c + 1) * size]
        pairs = [(int(order[c * size + int(rng.integers(0, k))]), int(order[c * size + k])) for c in range(count) for k in range(1, size)]
        bad = [(int(order[c * size]), int(order[(c + 1) * size])) for c in range(count - 1)]
    else:
        raise KeyError(name)
    pairs = _shuffled(rng, pairs)
    scores = np.tile(np.array(PASS, dtype=np.uint32), (len(pairs), 1))
    if bad:
        at = rng.integers(0, len(pairs) + 1, size=len(bad))
        pairs = np.insert(pairs, at, np.array(bad, dtype=np.uint32), axis=0)
        scores = np.insert(scores, at, np.array([(1, 100)] * len(bad), dtype=np.uint32), axis=0)
    if name == "two_joined_last":
        pairs = np.concatenate([pairs, np.array([[n - 1, n // 2 - 1]], dtype=np.uint32)])
        scores = np.concatenate([scores, np.array([PASS], dtype=np.uint32)])
    return n, pairs, scores, DEFAULT


@functools.lru_cache(maxsize=None)
def expected_link(name, small=False):
    n, pairs, scores, params = contention(name, small) if name in CONTENTION else link_cases()[name]
    labels, n_clusters, n_linked, n_invalid = C.link(n, [tuple(p) for p in np.asarray(pairs, dtype=np.uint64).reshape(-1, 2).tolist()],
                                                     np.asarray(scores, dtype=np.uint64).reshape(-1, 2).tolist(), params)
    return np.array(labels, dtype=np.uint64), n_clusters, n_linked, n_invalid


# ---- planted families ----------------------------------------------------------------------------------------------------------
FAMILY_SEED = 31
FAMILY_PARAMS = dict(k=21, log2_bins=8, n_bands=64, band_bins=2, min_similarity=0.2, min_filled=8)


def mutated(rng, s, sub=0.01):
    t = bytearray(s)
    for p in np.flatnonzero(rng.random(len(t)) < sub):
        t[p] = b"ACGT"[(b"ACGT".index(t[p]) + int(rng.integers(1, 4))) % 4]
    r = int(rng.integers(0, len(t)))
    t = bytes(t[r:] + t[:r])
    return R.revcomp(t) if rng.integers(0, 2) else t


@functools.lru_cache(maxsize=None)
def families(seed=FAMILY_SEED):
    """(records, family): 40 founders of 300 .. 1500 symbols, each with three copies at 1 % substitutions, a random rotation and a
    random strand, and 80 unrelated records, all shuffled; family[i] = the family of record i (an unrelated record is its own)."""
    rng = np.random.default_rng(seed)
    recs, fam = [], []
    for f in range(40):
        s = SS.random_acgt(rng, rng.integers(300, 1501))
        recs += [s] + [mutated(rng, s) for _ in range(3)]
        fam += [f] * 4
    for u in range(80):
        recs.append(SS.random_acgt(rng, rng.integers(300, 1501)))
        fam.append(40 + u)
    order = rng.permutation(len(recs))
    return tuple(recs[i] for i in order), tuple(fam[i] for i in order)


@functools.lru_cache(maxsize=None)
def families_expected(min_similarity=0.2, seed=FAMILY_SEED):
    """The yardstick over the planted set: (rows, offsets, pairs, scores, labels, n_clusters, n_linked)."""
    records, _ = families(seed)
    p = FAMILY_PARAMS
    rows, _ = SS.expected(records, p["k"], p["log2_bins"])
    offsets, pairs = C.candidates([[int(v) for v in row] for row in rows], p["n_bands"], p["band_bins"])
    match, filled, bad = R.compare_pairs(rows, rows, pairs)
    assert bad == 0
    scores = np.stack([match, filled], axis=1)
    labels, n_clusters, n_linked, n_invalid = C.link(len(records), pairs, scores.tolist(), (C.q16(min_similarity), p["min_filled"]))
    assert n_invalid == 0
    return rows, np.array(offsets, dtype=np.uint64), np.array(pairs, dtype=np.uint32).reshape(-1, 2), scores.astype(np.uint32), \
        np.array(labels, dtype=np.uint64), n_clusters, n_linked


def family_labels(family):
    """What the labels must be: the smallest index of every record's planted family."""
    first = {}
    for i, f in enumerate(family):
        first.setdefault(f, i)
    return np.array([first[f] for f in family], dtype=np.uint64)
