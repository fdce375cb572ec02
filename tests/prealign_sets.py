"""The input sets of the prealign unit, shared by the CPU fiber test (tests/test_prealign_cpu.py) and the GPU test
(tests/test_prealign_gpu.py).  TEST INFRASTRUCTURE ONLY.  Everything is seeded; the sizes follow the constants read from the
sources, as tests/grid_sets.py's do.

  anchor_cases()   name -> (records, k, log2_bins, seed, lead): `lead` junk bytes in front of the payload (offsets[0] != 0)
  vote_cases()     name -> (rows, anchors, lengths, k, min_votes, pairs): rows and anchors crafted directly
  planted()        founders and mutated copies with their recorded rotation, strand and substitutions
"""
import functools
import random

import numpy as np

from tests import grid_sets as G
from tests import prealign_ref as P
from tests import sketch_ref as R

EMPTY, NONE = P.EMPTY, P.NONE


@functools.lru_cache(maxsize=None)
def constants():
    c = dict(G.grid_constants())
    for name in ("PAIRS_MAX_GRID", "LABELS_WG", "LABELS_MAX_GRID"):
        c[name] = G._value(G._src("circkit_prealign.hip"), name)
    c["PREALIGN_WAVES"] = G._value(G._src("prealign.h"), "PREALIGN_WAVES")
    return c


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def rotate(s, r):
    r %= max(len(s), 1)
    return s[r:] + s[:r]


# ---- anchors ---------------------------------------------------------------------------------------------------------------------
def _wrapping_record(k, log2_bins):
    """A record one of whose bins is won by a k-mer that starts in the last k - 1 positions (it wraps round the end)."""
    for seed in range(1000):
        s = rand_seq(random.Random(7000 + seed), 40)
        _, _, anc = P.anchors(s, k, log2_bins)
        if any(a != NONE and (a >> 1) > len(s) - k for a in anc):
            return s
    raise AssertionError("no wrapping winner found")


@functools.lru_cache(maxsize=None)
def anchor_cases():
    c = constants()
    seg = c["SKETCH_SEG"]
    rng = random.Random(20240601)
    cases = {}
    k = 11
    lengths = [k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, seg - 1, seg, seg + 1, 2 * seg + 1, 3 * seg + 1]
    cases["lengths"] = ([rand_seq(rng, n) for n in lengths], k, 6, 0, 0)
    unit = rand_seq(rng, 7)
    base = rand_seq(rng, 50)
    cases["ties"] = ([unit * 40, base + base, base], 5, 4, 3, 0)          # every k-mer ties: the smallest start wins
    cases["wrap"] = ([_wrapping_record(8, 4)], 8, 4, 0, 0)
    cases["palindrome"] = ([b"TTACGCGTAAGG", b"ACGCGT", b"ACGCGTACGCGT"], 6, 4, 0, 0)       # ACGCGT is its own reverse complement
    cases["no_kmers"] = ([b"N" * 50, b"".join(rand_seq(rng, 7) + b"N" for _ in range(9)), b"", b"ACG"], 8, 4, 0, 0)
    cases["lead"] = ([rand_seq(rng, n) for n in (45, 0, 70, seg + 9)], 9, 5, 11, 13)
    cases["k4"] = ([rand_seq(rng, n) for n in (4, 5, 90)], 4, 4, 0, 0)
    cases["k32"] = ([rand_seq(rng, n) for n in (31, 32, 33, 200)], 32, 5, 2 ** 63 + 5, 0)
    cases["bins1024"] = ([rand_seq(rng, n) for n in (1500, 60)] + [rand_seq(rng, 900, b"ACGTN")], 15, 10, 0, 0)
    span_unit = rand_seq(rng, 3000)
    cases["two_spans"] = ([span_unit * 3, rotate(R.revcomp(span_unit * 3), 1234)], 13, 5, 0, 0)     # every bin's minimum lies in several spans
    return cases


@functools.lru_cache(maxsize=None)
def anchor_grid_cases():
    """One record past each fixed grid of the anchors build (the card only: too many records for the fibers)."""
    c = constants()
    rng = random.Random(77)
    few = [rand_seq(rng, 24) for _ in range(5)]
    n_short = c["SHORT_MAX_GRID"] * c["SKETCH_WAVES"] + 1
    longs = [rand_seq(rng, c["SKETCH_SEG"] + 1), rand_seq(rng, c["SKETCH_SEG"] + 40)]
    n_long = c["LONG_GRID"] + 1
    return {"past_short_grid": ([few[i % 5] for i in range(n_short)], 8, 4, 0, 0),
            "past_long_grid": ([longs[i % 2] for i in range(n_long)] + [few[0]], 12, 4, 0, 0)}


@functools.lru_cache(maxsize=None)
def expected_anchors(name):
    cases = anchor_cases()
    seqs, k, lb, seed, _ = cases[name] if name in cases else anchor_grid_cases()[name]
    return P.anchors_batch(seqs, k, lb, seed)


def csr(seqs, lead=0):
    """(payload with `lead` junk bytes in front, offsets)"""
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    data = np.frombuffer(b"\x07" * lead + b"".join(seqs), dtype=np.uint8).copy()
    return data, offsets + np.uint64(lead)


# ---- votes -----------------------------------------------------------------------------------------------------------------------
def anchor_pair(n_b, k, pa, s, start, oa=0):
    """(anchor of a, anchor of b) of a bin that votes (s, start) against a record of n_b symbols."""
    pb = (pa + start) % n_b
    if s:
        pb = (n_b - k - pb) % n_b
    return 2 * pa + oa, 2 * pb + (oa ^ s)


def craft(bins, n_a, n_b, k, votes):
    """Two records whose bin i holds votes[i] = (pa, s, start[, oa]) or None (an empty bin on both sides)."""
    rows = np.full((2, bins), EMPTY, dtype=np.uint64)
    anc = np.full((2, bins), NONE, dtype=np.uint32)
    for i, v in enumerate(votes):
        if v is None:
            continue
        rows[:, i] = (i << 54) | (1000 + i)
        anc[0, i], anc[1, i] = anchor_pair(n_b, k, *v)
    return rows, anc, np.array([n_a, n_b], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def vote_cases():
    cases = {}
    AB = [(0, 1)]
    pad = [None] * 10
    cases["tie_two_keys"] = craft(16, 80, 50, 8, [(3, 0, 5), (9, 0, 2), (1, 0, 5), (60, 0, 2), (7, 0, 5), (2, 0, 2)] + pad) + (8, 1, AB)
    cases["tie_strands"] = craft(16, 80, 50, 8, [(3, 1, 1), (9, 0, 9), (1, 1, 1), (60, 0, 9, 1), (7, 1, 1, 1), (2, 0, 9)] + pad) + (8, 1, AB)
    cases["all_distinct"] = craft(16, 100, 100, 8, [(i, i & 1, 90 - 3 * i) for i in range(16)]) + (8, 1, AB)
    cases["one_key_16"] = craft(16, 64, 64, 8, [(i * 5, 1, 17) for i in range(16)]) + (8, 16, AB)
    cases["one_key_1024"] = craft(1024, 5000, 4000, 21, [(i * 3, 0, 3999) for i in range(1024)]) + (21, 1024, AB)
    six = craft(16, 80, 50, 8, [(i, 0, 7) for i in range(6)] + [(i, 1, 30 + i) for i in range(4)] + [None] * 6)
    cases["votes_eq_min"] = six + (8, 6, AB)
    cases["votes_below_min"] = six + (8, 7, AB)
    cases["pa_exceeds_nb"] = craft(16, 9000, 100, 8, [(5000 + 7 * i, i & 1, 42) for i in range(16)]) + (8, 4, AB)
    cases["nb_eq_k"] = craft(16, 40, 8, 8, [(i, i % 3 == 0, 3) for i in range(16)]) + (8, 2, AB)
    cases["nb_zero"] = craft(16, 40, 7, 8, [(i, 0, 3) for i in range(16)])[:2] + (np.array([40, 0], dtype=np.uint64), 8, 1, AB + [(1, 0)])
    cases["nb_too_long"] = craft(16, 40, 7, 8, [(i, 0, 3) for i in range(16)])[:2] + (np.array([40, 2 ** 31], dtype=np.uint64), 8, 1, AB + [(1, 0)])
    rows, anc, lengths = craft(16, 80, 50, 8, [(i, 0, 7) for i in range(8)] + [(i, 0, 9) for i in range(8)])
    anc[0, 0:3] = NONE                                       # a NONE anchor under a filled bin, on either side
    anc[1, 2:5] = NONE
    cases["none_anchor"] = (rows, anc, lengths, 8, 1, AB + [(1, 0)])
    # a row of 1024 bins with arbitrary anchors against a short record: long runs, many keys, the network at full width
    rng = np.random.RandomState(5)
    rows = np.repeat(((np.arange(1024, dtype=np.uint64) << np.uint64(54)) | np.uint64(77))[None, :], 3, axis=0)
    rows[2, ::3] = EMPTY
    anc = rng.randint(0, 2 ** 32, size=(3, 1024), dtype=np.uint64).astype(np.uint32)
    anc[anc == NONE] = 0
    cases["random_1024"] = (rows, anc, np.array([2 ** 31 - 1, 37, 2 ** 31 - 1], dtype=np.uint64), 32, 3,
                            [(0, 1), (1, 0), (0, 2), (2, 1), (1, 1), (2, 2)])
    # every rotation and both strands of one record, real sketches
    base = rand_seq(random.Random(60), 60)
    seqs = [rotate(base, r) for r in range(60)] + [rotate(R.revcomp(base), r) for r in range(60)]
    rows, _, anc = P.anchors_batch(seqs, 8, 5)
    lengths = np.full(120, 60, dtype=np.uint64)
    cases["rotations"] = (rows, anc, lengths, 8, 4, [(0, i) for i in range(120)] + [(i, 0) for i in range(0, 120, 7)])
    cases["self_pairs"] = (rows[:9], anc[:9], lengths[:9], 8, 4, [(i, i) for i in range(9)])
    cases["invalid"] = (rows[:4], anc[:4], lengths[:4], 8, 4, [(0, 1), (4, 1), (1, 4), (2 ** 32 - 1, 0), (3, 2 ** 32 - 1), (7, 9), (2, 3)])
    cases["no_records"] = (rows[:0], anc[:0], lengths[:0], 8, 4, [(0, 0), (1, 0)])
    cases["no_pairs"] = (rows[:4], anc[:4], lengths[:4], 8, 4, [])
    return cases


@functools.lru_cache(maxsize=None)
def past_the_pairs_grid():
    """One pair more than the pairs kernel has waves (the card only)."""
    c = constants()
    rows, anc, lengths, k, mv, _ = vote_cases()["rotations"]
    m = c["PAIRS_MAX_GRID"] * c["PREALIGN_WAVES"] + 1
    pairs = [(i % 11, (i * 7) % 120) for i in range(m)]
    pairs[-1] = (1, 119)
    return rows, anc, lengths, k, mv, pairs


@functools.lru_cache(maxsize=None)
def expected_votes(name):
    rows, anc, lengths, k, mv, pairs = past_the_pairs_grid() if name == "past_the_pairs_grid" else vote_cases()[name]
    if name != "past_the_pairs_grid":
        return P.pairs(rows, anc, lengths, k, mv, pairs)
    seen = {}
    for a, b in pairs:                                       # few distinct pairs: each one once
        if (a, b) not in seen:
            seen[(a, b)] = P.pair(rows[a], anc[a], rows[b], anc[b], int(lengths[b]), b, k, mv)
    windows = np.array([seen[p][0] for p in pairs], dtype=P.WINDOW_DTYPE)
    scores = np.array([seen[p][1] for p in pairs], dtype=np.uint32)
    return windows, scores, sum(seen[p][2] for p in pairs), 0


def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
    return off


def label_cases():
    c = constants()
    past = c["LABELS_WG"] * c["LABELS_MAX_GRID"] + 1
    return {"plain": np.array([0, 0, 2, 1, 2 ** 32 - 1], dtype=np.uint64),
            "wide": np.array([0, 2 ** 32, 2 ** 32 + 1, 2 ** 64 - 1, 3], dtype=np.uint64),
            "empty": np.zeros(0, dtype=np.uint64),
            "past_the_labels_grid": (np.arange(past, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(past)}


# ---- planted ---------------------------------------------------------------------------------------------------------------------
PLANTED_SEED = 1


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED, n_founders=40, copies=3, rate=0.01):
    """(records, plants): 40 founders of 300 .. 1500 symbols, each followed by three copies with 1 % substitutions at a recorded
    rotation and strand.  plants: [(founder index, copy index, rotation r, strand s, substituted positions of the founder)]; the
    copy is rotate(S, r) with S the mutated founder (s = 0) or its reverse complement (s = 1)."""
    rng = random.Random(seed)
    records, plants = [], []
    for _ in range(n_founders):
        f = rand_seq(rng, rng.randint(300, 1500))
        fi = len(records)
        records.append(f)
        for _ in range(copies):
            m = bytearray(f)
            subs = sorted(rng.sample(range(len(f)), max(1, round(rate * len(f)))))
            for p in subs:
                m[p] = rng.choice([c for c in b"ACGT" if c != f[p]])
            r, s = rng.randrange(len(f)), rng.randrange(2)
            m = bytes(m)
            records.append(rotate(R.revcomp(m) if s else m, r))
            plants.append((fi, len(records) - 1, r, s, subs))
    return records, plants


def planted_window(n, r, s):
    """(start, strand) of the window on the copy that puts the founder's position 0 first."""
    return (r % n, 1) if s else ((n - r) % n, 0)
