"""The input sets of the distance unit, shared by the CPU fiber test (tests/test_distance_cpu.py) and the GPU test
(tests/test_distance_gpu.py).  TEST INFRASTRUCTURE ONLY.  Everything is seeded; the sizes follow the constants read from the
sources, as tests/prealign_sets.py's do.

  cases()        name -> Case: two batches (or one), a cutoff W, the pairs, which outputs are asked for
  expected(name) the yardstick's (distance, scores, n_within, n_invalid), computed once
A Case's batches are final: `data_a` is the payload with its lead bytes, `off_a` the offsets as the call gets them.
"""
import functools
import random

import numpy as np

from tests import distance_ref as D
from tests import grid_sets as G

OVER = D.OVER


@functools.lru_cache(maxsize=None)
def constants():
    c = {}
    for name in ("DISTANCE_WAVES", "SLICE_WORDS", "STAGE_SLACK", "DISTANCE_MAX"):
        c[name] = G._value(G._src("distance.h"), name)
    c["DISTANCE_MAX_GRID"] = G._value(G._src("circkit_distance.hip"), "DISTANCE_MAX_GRID")
    return c


def row_words(W):
    """distance.h's: the words of one row of diagonals."""
    return (2 * W + 3 + 3) & ~3


def stage_bytes(W):
    return 4 * (constants()["SLICE_WORDS"] - 2 * row_words(W))


def staged(n_x, n_y, W):
    """Whether the kernel copies the pair into LDS (distance.h's condition restated)."""
    return n_x + n_y + constants()["STAGE_SLACK"] <= stage_bytes(W)


def stage_limit(W):
    """The largest n_x + n_y that is staged."""
    return stage_bytes(W) - constants()["STAGE_SLACK"]


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def rotate(s, r):
    r %= max(len(s), 1)
    return s[r:] + s[:r]


def substitute(rng, s, count, alphabet=b"ACGT", at=None):
    m = bytearray(s)
    for p in (at if at is not None else rng.sample(range(len(s)), count)):
        m[p] = rng.choice([c for c in alphabet if c != s[p]])
    return bytes(m)


def mark(rng, s, count, byte=b"N"):
    """s with `count` symbols replaced by a byte that s does not hold: each costs one edit whatever the alignment, so lev = count."""
    assert byte not in s
    m = bytearray(s)
    for p in rng.sample(range(len(s)), count):
        m[p] = byte[0]
    return bytes(m)


def edit(rng, s, n_sub, n_ins, n_del, alphabet=b"ACGT"):
    """s with n_sub substitutions, n_ins insertions and n_del deletions at random places (as far as the record has room)."""
    m = bytearray(s)
    for _ in range(n_sub):
        if m:
            p = rng.randrange(len(m))
            m[p] = rng.choice([c for c in alphabet if c != m[p]])
    for _ in range(n_ins):
        m.insert(rng.randrange(len(m) + 1), rng.choice(alphabet))
    for _ in range(n_del):
        if m:
            del m[rng.randrange(len(m))]
    return bytes(m)


class Case:
    def __init__(self, a, b, W, pairs, lead_a=0, lead_b=0, out="both", off_a=None, off_b=None, len_a=None, len_b=None, tail_a=0, tail_b=0):
        self.a, self.b, self.W, self.pairs, self.out = list(a), (None if b is None else list(b)), W, [(int(i), int(j)) for i, j in pairs], out
        self.len_a, self.len_b = len_a, len_b
        self.data_a, self.off_a = self._csr(self.a, lead_a, off_a, tail_a)
        if b is None:
            self.data_b, self.off_b = self.data_a, self.off_a
        else:
            self.data_b, self.off_b = self._csr(self.b, lead_b, off_b, tail_b)

    @staticmethod
    def _csr(seqs, lead, off, tail):
        """(payload: `lead` junk bytes, the records, `tail` junk bytes that no record names; offsets, with crafted ones in place)"""
        offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        offsets += np.uint64(lead)
        if off is not None:
            offsets = np.asarray(off, dtype=np.uint64).copy()
        return np.frombuffer(b"\x07" * lead + b"".join(seqs) + b"\x4e" * tail, dtype=np.uint8).copy(), offsets

    @property
    def same(self):
        return self.b is None


def _aligned_copies(seq, fill=b"T"):
    """A batch that holds `seq` eight times, the copies at payload offsets 0 .. 7 mod 8 in turn (fillers in between): the records
    and the indices of the copies."""
    records, at, where = [], 0, []
    for want in range(8):
        pad = (want - at) % 8
        if pad or want == 0:
            records.append(fill * pad)
            at += pad
        where.append(len(records))
        records.append(seq)
        at += len(seq)
    return records, where


@functools.lru_cache(maxsize=None)
def cases():
    rng = random.Random(20250607)
    out = {}

    # ---- lengths ----
    W = 8
    a = [b"", b"", b"", b"", b"G", b"G"] + [rand_seq(rng, n) for n in (7, 8, 9, 63, 64, 65, 511, 512, 513)]
    b = [b"", rand_seq(rng, W - 1), rand_seq(rng, W), rand_seq(rng, W + 1), b"G", b"C"] + a[6:]
    out["lengths"] = Case(a, b, W, [(i, i) for i in range(len(a))] + [(1, 0), (2, 1), (3, 2), (6, 7), (7, 8), (9, 10), (12, 13), (13, 14)])
    lim = stage_limit(W)
    half = lim // 2
    base = rand_seq(rng, half + 2)
    near = [edit(rng, base[:n], 2, 1, 1)[:n] for n in (half, half, half + 1)]
    near = [s + rand_seq(rng, n - len(s)) for s, n in zip(near, (half, half, half + 1))]
    #   n_x + n_y = limit - 1, limit, limit + 1 (the last one on the global path), and one pair far on the global path
    far = rand_seq(rng, lim)
    out["stage_limit"] = Case([base[:lim - 1 - half], base[:lim - half], base[:lim - half], far], near + [edit(rng, far, 3, 2, 2)], W,
                              [(0, 0), (1, 1), (2, 2), (3, 3)])

    # ---- placement ----
    for name, n, W in (("placement_tail", 37, 6), ("placement_whole", 150, 6), ("placement_global", 500, 255)):
        x = rand_seq(rng, n)
        y = edit(rng, x, 2, 1, 0)
        ra, wa = _aligned_copies(x)
        rb, wb = _aligned_copies(y, b"G")
        out[name] = Case(ra, rb, W, [(i, j) for i in wa for j in wb], lead_a=3, lead_b=5)
    for name, n in (("differ_short", 40), ("differ_long", 700)):
        x = rand_seq(rng, n)
        ys = [substitute(rng, x, 1, at=[p]) for p in (0, n - 1, 7, 8, 9)]
        out[name] = Case([x], ys, 2, [(0, j) for j in range(5)], lead_a=1, lead_b=2)

    # ---- the cutoff ----
    def cutoff_case(W, n=300, gaps=True):
        x = rand_seq(rng, n)
        ys = [mark(rng, x, k) for k in (max(W - 1, 0), W, W + 1)]
        if gaps:
            ys += [rand_seq(rng, W) + x, rand_seq(rng, W + 1) + x, x + rand_seq(rng, W), x + rand_seq(rng, W + 1)]
        return Case([x], ys, W, [(0, j) for j in range(len(ys))])
    out["cutoff_8"] = cutoff_case(8)
    for W in (0, 1, 31, 32, 33, 63, 64):
        out["cutoff_%d" % W] = cutoff_case(W)
    x = rand_seq(rng, 600)
    ys = [edit(rng, x, k - 2 * (k // 6), k // 6, k // 6) for k in (230, 250, 255, 256, 262, 275)] + [substitute(rng, x, k) for k in (250, 270)]

    def marked(k, n_ins):
        """lev = k + n_ins exactly: k symbols marked, n_ins marks inserted"""
        m = bytearray(mark(rng, x, k))
        for _ in range(n_ins):
            m.insert(rng.randrange(len(m) + 1), ord("N"))
        return bytes(m)
    ys += [marked(248, 7), marked(249, 7), marked(260, 0), marked(254, 0), marked(255, 0), marked(256, 0)]
    out["cutoff_255"] = Case([x], ys, 255, [(0, j) for j in range(len(ys))])
    #   a length gap of W + 1: record 1 of A is named by offsets that point behind every record, into bytes that nobody may read
    W = 8
    x = rand_seq(rng, 50)
    off = np.array([0, 50, 50, 50 + 16, 50 + 16 + 50 + W + 1], dtype=np.uint64)     # record 3: 59 symbols of the tail
    out["gap_unread"] = Case([x, b"", b"", b""], None, W, [(0, 3), (3, 0), (0, 0), (1, 3)], off_a=off, len_a=[50, 0, 16, 59], tail_a=16 + 59)

    # ---- repeats ----
    W = 12
    a, b = [], []
    a.append(b"A" * 50); b.append(b"A" * 51)
    for unit in (b"AC", b"ACG"):
        t = unit * 40
        a += [t, t, t]
        b += [t[:31] + t[32:], t[:17] + t[18:61] + t[62:], t[:20] + b"A" + t[20:70] + t[71:]]
    r = rand_seq(rng, 200)
    for k in range(1, 6):
        a.append(r); b.append(rotate(r, k))
    a.append(b"ACGTACGT"); b.append(b"CGTACGTA")
    out["repeats"] = Case(a, b, W, [(i, i) for i in range(len(a))])

    # ---- bytes ----
    odd = bytes([0x00, 0xFF, ord("N"), ord("-"), ord("a"), ord("A"), ord("c"), ord("C")])
    x = rand_seq(rng, 100, odd)
    a = [b"ACGN", b"acgt", b"\x00\x00\xff", b"N", b"a", b"A-C-G", x, x]
    b = [b"ACGN", b"ACGT", b"\xff\x00\xff", b"N", b"A", b"AC-G-", edit(rng, x, 3, 1, 1, odd), bytes(ch ^ 0x20 if chr(ch).isalpha() else ch for ch in x)]
    out["bytes"] = Case(a, b, 40, [(i, i) for i in range(len(a))])
    out["bytes_low_cutoff"] = Case(a, b, 3, [(i, i) for i in range(len(a))])

    # ---- random: 300 pairs, each with a cutoff of its own, one call per cutoff ----
    #   (a generator of its own: with these ranges about a third of the pairs comes out OVER, and the CPU test asserts that at
    #   least a third does; the seed is one for which the yardstick says so)
    by_w = {}
    rng_set, rng = rng, random.Random(7)
    for _ in range(300):
        x = rand_seq(rng, rng.randrange(301))
        k = rng.randrange(41)
        n_sub = rng.randrange(k + 1)
        n_ins = rng.randrange(k - n_sub + 1)
        y = edit(rng, x, n_sub, n_ins, k - n_sub - n_ins)
        by_w.setdefault(rng.randrange(49), []).append((x, y))
    rng = rng_set
    for W, xy in sorted(by_w.items()):
        out["random_%02d" % W] = Case([x for x, _ in xy], [y for _, y in xy], W, [(i, i) for i in range(len(xy))])

    # ---- pairs ----
    recs = [rand_seq(rng, n) for n in (30, 31, 0, 100, 100, 64)]
    recs[4] = substitute(rng, recs[3], 4)
    others = [edit(rng, s, 1, 1, 0) for s in recs[:4]]
    out["self_pairs"] = Case(recs, None, 5, [(i, i) for i in range(len(recs))] + [(3, 4), (4, 3), (0, 1)])
    out["two_batches"] = Case(recs, others, 5, [(i, i) for i in range(4)] + [(0, 1), (5, 3)])
    out["duplicates"] = Case(recs, others, 5, [(3, 3), (3, 3), (0, 0), (3, 3), (0, 0)])
    out["invalid"] = Case(recs, others, 5, [(0, 0), (6, 0), (0, 4), (2 ** 32 - 1, 1), (1, 2 ** 32 - 1), (9, 9), (3, 3)])
    #   a record of 2^31 symbols by its offsets alone, on either side: never dereferenced
    long_a = np.array([0, 30, 30 + 2 ** 31, 30 + 2 ** 31 + 5], dtype=np.uint64)
    out["too_long_a"] = Case([recs[0], b"", b""], others, 5, [(0, 0), (1, 0), (1, 1), (0, 0)], off_a=long_a, len_a=[30, 2 ** 31, 5])
    n0 = len(others[0])
    long_b = np.array([4, 4 + n0, 4 + n0 + 2 ** 31 + 7, 4 + n0 + 2 ** 31 + 7 + 3], dtype=np.uint64)
    out["too_long_b"] = Case(recs, [others[0], b"", b""], 5, [(0, 0), (0, 1), (2, 1), (3, 1), (0, 0)], lead_b=4, off_b=long_b, len_b=[n0, 2 ** 31 + 7, 3])
    out["only_distance"] = Case(recs, others, 5, [(i, i) for i in range(4)] + [(9, 0)], out="distance")
    out["only_scores"] = Case(recs, others, 5, [(i, i) for i in range(4)] + [(9, 0)], out="scores")
    out["no_pairs"] = Case(recs, others, 5, [])
    out["no_records"] = Case([], None, 5, [(0, 0), (1, 0)])
    return out


@functools.lru_cache(maxsize=None)
def past_the_grid():
    """One pair more than the pairs kernel has waves (the card only): few distinct pairs, the last one of its own."""
    c = constants()
    rng = random.Random(99)
    recs = [rand_seq(rng, n) for n in (40, 41, 39, 40, 90)]
    recs[3] = substitute(rng, recs[0], 3)
    m = c["DISTANCE_MAX_GRID"] * c["DISTANCE_WAVES"] + 1
    pairs = [(i % 4, (i * 3) % 4) for i in range(m)]
    pairs[-1] = (4, 4)
    pairs[-2] = (0, 3)
    return Case(recs, None, 6, pairs)


@functools.lru_cache(maxsize=None)
def planted():
    """tests/prealign_sets.py's planted families, each copy cut by the window the YARDSTICK prealign finds for (founder, copy): a
    Case at W = 64 whose batch A holds the records and whose batch B holds the cut windows, pair p = (founder, p); and the planted
    substitution counts."""
    from tests import prealign_ref as P
    from tests import prealign_sets as PS
    records, plants = PS.planted()
    k, lb, mv = 21, 8, 4
    rows, _, anc = P.anchors_batch(records, k, lb)
    cut, pairs, counts = [], [], []
    for fi, ci, _, _, subs in plants:
        w, _, aligned = P.pair(rows[fi], anc[fi], rows[ci], anc[ci], len(records[ci]), ci, k, mv)
        assert aligned
        cut.append(P.window_bytes(records, np.array([w], dtype=P.WINDOW_DTYPE)[0]))
        pairs.append((fi, len(cut) - 1))
        counts.append(len(subs))
    return Case(records, cut, 64, pairs), counts


@functools.lru_cache(maxsize=None)
def expected(name):
    case = past_the_grid() if name == "past_the_grid" else planted()[0] if name == "planted" else cases()[name]
    return D.pairs(case.a, case.b, case.pairs, case.W, case.len_a, case.len_b if not case.same else case.len_a)
