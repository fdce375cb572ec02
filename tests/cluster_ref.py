"""The yardstick of the cluster unit (TEST INFRASTRUCTURE ONLY): the definition of include/circkit.h's "clusters of circular
records" restated with Python integers, dicts and lists, on top of tests/sketch_ref.py.  It is not the code under test: the
representative of a key is a dict lookup, the clusters are found by merging Python sets."""
from tests import sketch_ref as R

MASK = R.MASK
EMPTY = R.EMPTY
NO_KEY = MASK
GOLDEN = 0x9e3779b97f4a7c15


def band_key(row, b, band_bins):
    """The key of band b of a row (a sequence of integers), or None where the band has none."""
    x = ((b + 1) * GOLDEN) & MASK
    for v in row[b * band_bins:(b + 1) * band_bins]:
        v = int(v)
        if v == EMPTY:
            return None
        x = R.fmix64(x ^ v)
    return None if x == NO_KEY else x


def candidates(rows, n_bands, band_bins):
    """(offsets, pairs): offsets a list of n + 1 integers, pairs a list of (rep, i), record i's in [offsets[i], offsets[i + 1])."""
    keys = [[band_key(row, b, band_bins) for b in range(n_bands)] for row in rows]
    rep = {}
    for i, ks in enumerate(keys):
        for k in ks:
            if k is not None and k not in rep:
                rep[k] = i
    offsets, pairs = [0], []
    for i, ks in enumerate(keys):
        proposed = []
        for k in ks:
            if k is not None and rep[k] < i and rep[k] not in proposed:
                proposed.append(rep[k])
        pairs += [(r, i) for r in proposed]
        offsets.append(len(pairs))
    return offsets, pairs


def links(match, filled, min_similarity_q16, min_filled):
    return filled >= min_filled and (int(match) << 16) >= min_similarity_q16 * int(filled)


def link(n, pairs, scores, params):
    """(labels, n_clusters, n_linked, n_invalid) of n records; params = (min_similarity_q16, min_filled); scores[p] = (match,
    filled) of pairs[p].  Merges sets: no parent array, no order."""
    q16, min_filled = params
    member = {i: {i} for i in range(n)}                   # record -> the set it belongs to (shared by its members)
    n_linked = n_invalid = 0
    for (i, j), (m, f) in zip(pairs, scores):
        i, j = int(i), int(j)
        if i >= n or j >= n:
            n_invalid += 1
            continue
        if i == j:
            continue
        if not links(int(m), int(f), q16, min_filled):
            continue
        n_linked += 1
        a, b = member[i], member[j]
        if a is b:
            continue
        if len(a) < len(b):
            a, b = b, a
        a |= b
        for x in b:
            member[x] = a
    smallest = {}                                         # one min() per set
    for s in member.values():
        if id(s) not in smallest:
            smallest[id(s)] = min(s)
    labels = [smallest[id(member[i])] for i in range(n)]
    return labels, sum(labels[i] == i for i in range(n)), n_linked, n_invalid


def q16(similarity):
    return int(round(similarity * 65536))
