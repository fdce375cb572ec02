"""The yardstick of the distance unit: the "edit distance of record pairs" section of include/circkit.h restated as the plain full
dynamic program.  TEST INFRASTRUCTURE ONLY: it imports nothing of the product, and tests/test_distance_cpu.py holds it against
answers written out by hand."""
import numpy as np

OVER = 0xFFFFFFFF
DISTANCE_MAX = 255
TOO_LONG = 1 << 31


def table(x, y):
    """The full (n_x + 1) x (n_y + 1) table of Levenshtein distances of the prefixes, Python integers."""
    x, y = bytes(x), bytes(y)
    t = [[0] * (len(y) + 1) for _ in range(len(x) + 1)]
    for j in range(len(y) + 1):
        t[0][j] = j
    for i in range(1, len(x) + 1):
        t[i][0] = i
        for j in range(1, len(y) + 1):
            t[i][j] = min(t[i - 1][j - 1] + (x[i - 1] != y[j - 1]), t[i - 1][j] + 1, t[i][j - 1] + 1)
    return t


def lev(x, y):
    """The Levenshtein distance with unit costs: the full table, a numpy row at a time.  Within a row the insertions are a running
    minimum: row[j] = min over j' <= j of (cand[j'] + j - j')."""
    x = np.frombuffer(bytes(x), dtype=np.uint8)
    y = np.frombuffer(bytes(y), dtype=np.uint8)
    idx = np.arange(len(y) + 1, dtype=np.int64)
    row = idx.copy()
    for i in range(len(x)):
        cand = np.empty(len(y) + 1, dtype=np.int64)
        cand[0] = i + 1
        cand[1:] = np.minimum(row[:-1] + (y != x[i]), row[1:] + 1)
        row = np.minimum.accumulate(cand - idx) + idx
    return int(row[-1])


def bounded(x, y, W):
    d = lev(x, y)
    return d if d <= W else OVER


def pairs(seqs_a, seqs_b, pair_list, W, lengths_a=None, lengths_b=None):
    """(distance uint32[m], scores uint32[m, 2], n_within, n_invalid) of the pairs (i, j) of two lists of records.  lengths_a /
    lengths_b: the lengths the offsets claim, where they differ from the records' (crafted offsets: a length of 2^31 or more)."""
    assert 0 <= W <= DISTANCE_MAX
    seqs_b = seqs_a if seqs_b is None else seqs_b
    la = [len(s) for s in seqs_a] if lengths_a is None else list(lengths_a)
    lb = [len(s) for s in seqs_b] if lengths_b is None else list(lengths_b)
    dist = np.zeros(len(pair_list), dtype=np.uint32)
    scores = np.zeros((len(pair_list), 2), dtype=np.uint32)
    within = invalid = 0
    seen = {}
    for p, (i, j) in enumerate(pair_list):
        if i >= len(la) or j >= len(lb) or la[i] >= TOO_LONG or lb[j] >= TOO_LONG:
            dist[p], invalid = OVER, invalid + 1
            continue
        L = max(la[i], lb[j])
        if (i, j) not in seen:
            seen[(i, j)] = OVER if abs(la[i] - lb[j]) > W else bounded(seqs_a[i], seqs_b[j], W)
        d = seen[(i, j)]
        dist[p] = d
        scores[p] = (0, L) if d == OVER else (L - d, L)
        within += d != OVER
    return dist, scores, within, invalid


def links(scores, min_similarity_q16, min_filled=1):
    """Whether each scored pair links, as circkit_cluster_link_device decides it."""
    s = np.asarray(scores, dtype=np.uint64).reshape(-1, 2)
    return (s[:, 1] >= min_filled) & ((s[:, 0] << np.uint64(16)) >= np.uint64(min_similarity_q16) * s[:, 1])
