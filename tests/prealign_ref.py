"""The yardstick of the prealign unit (TEST INFRASTRUCTURE ONLY): the definition of include/circkit.h's "pre-alignment of circular
records" restated with Python integers: the anchors by one loop per start (the digit reading is tests/sketch_ref.py's), the vote
with a Counter, the window as a tuple.  It imports nothing of the product."""
from collections import Counter

import numpy as np

from tests import sketch_ref as R

NONE = 0xFFFFFFFF
EMPTY = R.EMPTY
TOO_LONG = R.TOO_LONG
WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])


def anchors(seq, k, log2_bins, seed=0):
    """(row, n_kmers, anchors) of one record: anchors[b] = 2 * p + o of the smallest start p whose valid k-mer has h == row[b],
    o = (r < f); NONE where row[b] is EMPTY."""
    seq = bytes(seq)
    n = len(seq)
    bins = 1 << log2_bins
    row, anc = [EMPTY] * bins, [NONE] * bins
    if n < k:
        return row, 0, anc
    fwd = seq.translate(R._DIGITS).decode()
    rev = fwd[::-1].encode().translate(R._COMPLEMENT).decode()
    fwd2, rev2 = fwd + fwd, rev + rev
    seen = []
    for p in range(n):
        w = fwd2[p:p + k]
        if "x" in w:
            continue
        q = (n - p - k) % n
        f, r = int(w, 4), int(rev2[q:q + k], 4)
        h = R.fmix64(min(f, r) ^ seed)
        seen.append((h, p, 1 if r < f else 0))
        b = h >> (64 - log2_bins)
        if h < row[b]:
            row[b] = h
    for h, p, o in seen:                                    # in ascending p: the first start with the bin's h stays
        b = h >> (64 - log2_bins)
        if h == row[b] and h != EMPTY and anc[b] == NONE:
            anc[b] = 2 * p + o
    return row, len(seen), anc


_CACHE = {}


def anchors_batch(seqs, k, log2_bins, seed=0):
    """(rows (n, bins) uint64, counts uint32, anchors (n, bins) uint32) of a list of records; equal records are computed once."""
    bins = 1 << log2_bins
    rows = np.empty((len(seqs), bins), dtype=np.uint64)
    counts = np.zeros(len(seqs), dtype=np.uint32)
    anc = np.empty((len(seqs), bins), dtype=np.uint32)
    for i, s in enumerate(seqs):
        s = bytes(s)
        if len(s) >= TOO_LONG:
            rows[i], anc[i] = EMPTY, NONE
            continue
        key = (s, k, log2_bins, seed)
        if key not in _CACHE:
            row, c, a = anchors(s, k, log2_bins, seed)
            _CACHE[key] = (np.array(row, dtype=np.uint64), c, np.array(a, dtype=np.uint32))
        rows[i], counts[i], anc[i] = _CACHE[key]
    return rows, counts, anc


def vote_keys(row_a, anc_a, row_b, anc_b, n_b, k):
    """(keys of the matching bins in bin order, matches).  No key when n_b is 0 or 2^31 and more."""
    keys, matches = [], 0
    for x, y, aa, ab in zip(row_a, row_b, anc_a, anc_b):
        x, y, aa, ab = int(x), int(y), int(aa), int(ab)
        if x != y or x == EMPTY or aa == NONE or ab == NONE:
            continue
        matches += 1
        if n_b == 0 or n_b >= TOO_LONG:
            continue
        pa, oa, pb, ob = aa >> 1, aa & 1, ab >> 1, ab & 1
        s = oa ^ ob
        if s == 1:
            pb = (n_b - pb - k) % n_b
        keys.append((s << 31) | ((pb - pa) % n_b))
    return keys, matches


def pair(row_a, anc_a, row_b, anc_b, n_b, b, k, min_votes):
    """((length, record, start, strand, 0), (votes, matches), aligned) of one valid pair."""
    keys, matches = vote_keys(row_a, anc_a, row_b, anc_b, n_b, k)
    votes, key = 0, 0
    for v, c in Counter(keys).items():
        if c > votes or (c == votes and v < key):
            votes, key = c, v
    if votes >= min_votes:
        return (n_b, b, key & 0x7FFFFFFF, key >> 31, 0), (votes, matches), True
    return (n_b, b, 0, 0, 0), (votes, matches), False


def pairs(rows, anc, lengths, k, min_votes, pair_list):
    """(windows WINDOW_DTYPE, scores (m, 2) uint32, n_aligned, n_invalid) over a list of pairs."""
    pair_list = np.asarray(pair_list, dtype=np.uint64).reshape(-1, 2)
    n = len(lengths)
    windows = np.zeros(len(pair_list), dtype=WINDOW_DTYPE)
    scores = np.zeros((len(pair_list), 2), dtype=np.uint32)
    n_aligned = n_invalid = 0
    for at, (a, b) in enumerate(pair_list):
        a, b = int(a), int(b)
        if a >= n or b >= n:
            windows[at] = (0, b, 0, 0, 0)
            n_invalid += 1
            continue
        w, sc, al = pair(rows[a], anc[a], rows[b], anc[b], int(lengths[b]), b, k, min_votes)
        windows[at], scores[at] = w, sc
        n_aligned += al
    return windows, scores, n_aligned, n_invalid


def pairs_of_labels(labels):
    """pair i = (labels[i], i), a label of 2^32 or more as 0xFFFFFFFF."""
    return np.array([(NONE if int(l) >> 32 else int(l), i) for i, l in enumerate(labels)], dtype=np.uint32).reshape(-1, 2)


def window_bytes(seqs, w):
    """The bytes circkit_windows_gather_device writes for a valid window: length symbols of the strand from start, cyclically."""
    s = bytes(seqs[int(w["record"])])
    if not s:
        return b""
    if int(w["strand"]):
        s = R.revcomp(s)
    n, st = len(s), int(w["start"]) % len(s)
    return bytes(s[(st + t) % n] for t in range(int(w["length"])))
