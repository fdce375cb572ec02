"""The cluster yardstick as array arithmetic (TEST INFRASTRUCTURE ONLY): band_keys and candidates of tests/cluster_ref.py in numpy
uint64, for input sets of millions of keys, which Python integers and dicts are too slow for.  It restates the definition of
include/circkit.h's "clusters of circular records", not the device code: the first holder of a key is the first index of
np.unique over a stable order of all keys, a record's repeated representatives fall to a sort by (record, representative).
tests/test_cluster_np_cpu.py holds it against tests/cluster_ref.py, exactly."""
import numpy as np

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
EMPTY = NO_KEY
GOLDEN = 0x9e3779b97f4a7c15
_S33 = np.uint64(33)
_M1, _M2 = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53)


def fmix64(h):
    """MurmurHash3's 64-bit finalizer over a uint64 array (the products wrap, as 64-bit products do)."""
    h = h ^ (h >> _S33)
    h = h * _M1
    h = h ^ (h >> _S33)
    h = h * _M2
    return h ^ (h >> _S33)


def band_keys(rows, n_bands, band_bins):
    """(n, n_bands) uint64: the key of every band, NO_KEY where the band holds an EMPTY bin (or the key came out as ~0)."""
    rows = np.asarray(rows, dtype=np.uint64)
    n = len(rows)
    seed = np.array([((b + 1) * GOLDEN) & 0xFFFFFFFFFFFFFFFF for b in range(n_bands)], dtype=np.uint64)
    x = np.broadcast_to(seed, (n, n_bands)).copy()
    empty = np.zeros((n, n_bands), dtype=bool)
    bands = rows[:, :n_bands * band_bins].reshape(n, n_bands, band_bins)
    for j in range(band_bins):
        v = bands[:, :, j]
        empty |= v == EMPTY
        x = fmix64(x ^ v)
    x[empty] = NO_KEY
    return x


def maybe_shared(flat):
    """The positions, ascending, of every key that another position holds too -- and of a few that none does: a superset, which
    is all the caller needs.  It exists for speed alone (21 M keys: an index sort takes seconds, a sort of values a fraction of
    one): the position replaces the key's low bits, one sort of these words brings keys with equal high bits together, and a
    word whose neighbour has the same high bits stays.  Equal keys have equal high bits, so none of them is lost."""
    n = len(flat)
    bits = max(1, (n - 1).bit_length())
    if bits > 32:
        return np.arange(n, dtype=np.int64)
    low = np.uint64((1 << bits) - 1)
    words = np.sort((flat & ~low) | np.arange(n, dtype=np.uint64))
    same = (words[1:] >> np.uint64(bits)) == (words[:-1] >> np.uint64(bits))
    stays = np.zeros(n, dtype=bool)
    stays[1:] |= same
    stays[:-1] |= same
    return np.sort(words[stays] & low).astype(np.int64)


def candidates(rows, n_bands, band_bins, keys=None, with_bands=False):
    """(offsets uint64[n + 1], pairs uint32[m, 2]): the pairs (rep, i) of record i in [offsets[i], offsets[i + 1]), in the order
    of the bands that first propose each rep.  keys: band_keys(rows, n_bands, band_bins) where the caller has them already.
    with_bands: a third result, the band that proposes each pair."""
    n = len(rows)
    if keys is None:
        keys = band_keys(rows, n_bands, band_bins)
    flat = keys.reshape(-1)
    # a key that one position alone holds proposes nothing and represents nobody: only the others go on (in position order)
    at = maybe_shared(flat)
    # the first holder of every key: np.unique sorts stably with return_index, so the index is the smallest position
    _, first, inverse = np.unique(flat[at], return_index=True, return_inverse=True)
    first_pos = at[first][inverse.reshape(-1)]
    proposes = (flat[at] != NO_KEY) & (first_pos // n_bands < at // n_bands)
    at, first_pos = at[proposes], first_pos[proposes]
    rec, band, rep = at // n_bands, at % n_bands, first_pos // n_bands
    # of a record's bands with one rep the first stays: by (record, rep, band), keep the head of each run, back to band order
    order = np.lexsort((band, rep, rec))
    rec, band, rep = rec[order], band[order], rep[order]
    head = np.ones(len(rec), dtype=bool)
    head[1:] = (rec[1:] != rec[:-1]) | (rep[1:] != rep[:-1])
    rec, band, rep = rec[head], band[head], rep[head]
    order = np.lexsort((band, rec))
    rec, band, rep = rec[order], band[order], rep[order]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(rec, minlength=n)[:n] if n else np.zeros(0, dtype=np.int64))
    pairs = np.stack([rep, rec], axis=1).astype(np.uint32).reshape(-1, 2)
    return (offsets, pairs, band) if with_bands else (offsets, pairs)
