"""Input sets of the sketch unit, shared by its CPU fiber test and its GPU test (TEST INFRASTRUCTURE ONLY).  Everything is seeded,
and the yardstick's answer for a set is computed once and kept."""
import functools
import os
import re

import numpy as np

from tests import sketch_ref as R

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
KS = (4, 5, 15, 16, 17, 21, 31, 32)
LOG2_BINS = (4, 6, 8, 10)
# not the full product: every k at 256 bins, every bin count at k = 21
USEFUL_SEED = 11                # of planted(): the yardstick alone holds the usefulness bounds under it (tests/test_sketch_cpu.py)
PARAMS = tuple((k, 8) for k in KS) + tuple((21, b) for b in LOG2_BINS if b != 8)


def constants():
    src = open(os.path.join(CSRC, "sketch.h")).read()
    c = {}
    for name in ("SKETCH_SEG", "SKETCH_WAVES"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, name
        c[name] = int(m.group(1))
    return c


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offs


def random_acgt(rng, n):
    return bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(n))])


def with_symbol(seq, positions, symbol=b"N"):
    s = bytearray(seq)
    for p in positions:
        s[p] = symbol[0]
    return bytes(s)


def lengths(k, seg=None):
    seg = seg or constants()["SKETCH_SEG"]
    return list(range(201)) + [255, 256, 257, 1023, 1024, 1025, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 3 * seg + k - 2] + [k - 1, k, k + 1]


@functools.lru_cache(maxsize=None)
def length_records(k, seg=None):
    """One record of every length of lengths(k); every seventh holds a few bytes outside ACGT."""
    rng = np.random.default_rng(100 + k)
    out = []
    for i, n in enumerate(lengths(k, seg)):
        s = random_acgt(rng, n)
        if i % 7 == 3 and n:
            s = with_symbol(s, rng.integers(0, n, size=1 + n // 300), b"N-acgtn"[i // 7 % 7:i // 7 % 7 + 1])
        out.append(s)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def symbol_records(k, seg=None):
    """What the symbols can do: (name, record) pairs."""
    seg = seg or constants()["SKETCH_SEG"]
    rng = np.random.default_rng(7)
    base = random_acgt(rng, 40)
    out = [("N at %d" % p, with_symbol(base, [p])) for p in range(40)]
    out += [("all N", b"N" * 50), ("dash", with_symbol(random_acgt(rng, 90), [0, 44, 89], b"-")), ("lower case", random_acgt(rng, 70).lower()),
            ("one lower", with_symbol(random_acgt(rng, 70), [33], b"a")), ("poly-A", b"A" * 100), ("poly-A short", b"A" * k),
            ("palindromes", b"ACGT" * 9 + b"AATT" + b"GAATTC" * 3 + random_acgt(rng, 30)),
            ("other bytes", with_symbol(random_acgt(rng, 120), [5, 50, 100], b"\x00") + b"U" + bytes([0xFF, 0x41 + 0x80]) + random_acgt(rng, 40))]
    long = random_acgt(rng, 2 * seg + 500)
    out += [("N before the boundary", with_symbol(long, [seg - 1])), ("N after the boundary", with_symbol(long, [seg])),
            ("N on both sides", with_symbol(long, [seg - 1, seg, 2 * seg - 1, 2 * seg])), ("N at the ends of a long record", with_symbol(long, [0, len(long) - 1]))]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(records, k, log2_bins, seed=0):
    """The yardstick over a tuple of records (kept: the sets are shared between tests)."""
    rows, counts = R.sketch_batch(records, k, log2_bins, seed)
    rows.setflags(write=False)
    counts.setflags(write=False)
    return rows, counts


def poly_a_seed_for_empty(k):
    """The seed under which the one canonical k-mer of a poly-A record (c = 0) hashes to 2^64 - 1."""
    return R.fmix64_inverse(R.EMPTY)


def planted(seed, n=60, sub=0.01):
    """n random records of 300 .. 1500 symbols, then each once more with `sub` substitutions, a random rotation and a random
    strand, then n unrelated ones.  Returns (records, planted pairs, unrelated pairs)."""
    rng = np.random.default_rng(seed)
    base = [random_acgt(rng, rng.integers(300, 1501)) for _ in range(n)]
    twins = []
    for s in base:
        t = bytearray(s)
        for p in np.flatnonzero(rng.random(len(t)) < sub):
            t[p] = b"ACGT"[(b"ACGT".index(t[p]) + int(rng.integers(1, 4))) % 4]
        r = int(rng.integers(0, len(t)))
        t = bytes(t[r:] + t[:r])
        twins.append(R.revcomp(t) if rng.integers(0, 2) else t)
    others = [random_acgt(rng, rng.integers(300, 1501)) for _ in range(n)]
    return tuple(base + twins + others), [(i, n + i) for i in range(n)], [(i, 2 * n + i) for i in range(n)] + [(n + i, 2 * n + (i + 1) % n) for i in range(n)]


def compare_rows(rng, log2_bins, n=24):
    """Rows for the compare: random ones, copies, disjoint ones, empty ones, half-filled ones."""
    bins = 1 << log2_bins
    rows = rng.integers(0, 2 ** 63, size=(n, bins), dtype=np.uint64)
    rows[1] = rows[0]                                       # identical
    rows[2] = rows[0] + np.uint64(1)                        # disjoint from 0
    rows[3] = np.uint64(R.EMPTY)                            # empty
    rows[4] = np.uint64(R.EMPTY)
    rows[5] = rows[0]
    rows[5, ::2] = np.uint64(R.EMPTY)                       # half of 0
    rows[6] = rows[0]
    rows[6, bins // 4:] = rng.integers(0, 2 ** 63, size=bins - bins // 4, dtype=np.uint64)
    rows[7, 1::3] = np.uint64(R.EMPTY)
    rows[7, 0] = rows[0, 0]
    rows[8, -1] = rows[0, -1]                               # the last bin alone matches
    return rows
