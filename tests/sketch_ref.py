"""The yardstick of the sketch unit (TEST INFRASTRUCTURE ONLY): the definition of include/circkit.h's "sketches of circular
records" restated with Python integers, one loop per start and no packing tricks.  It is not the code under test: the k-mer at
start p is read as a number in base 4 from the record written twice, its reverse complement from the reverse complement written
twice, and Python's int() does the positional arithmetic."""
import numpy as np

MASK = 2 ** 64 - 1
EMPTY = MASK
TOO_LONG = 2 ** 31

# A C G T -> the digits 0 1 2 3; every other byte -> 'x', which no number holds
_DIGITS = bytes(ord("0123"["ACGT".index(chr(b))]) if chr(b) in "ACGT" else ord("x") for b in range(256))
_COMPLEMENT = bytes.maketrans(b"0123", b"3210")


def fmix64(h):
    """MurmurHash3's 64-bit finalizer."""
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & MASK
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & MASK
    h ^= h >> 33
    return h


def _unxorshift33(h):
    return h ^ (h >> 33)                       # (33 >= 32: the shifted part is untouched, one step inverts)


def fmix64_inverse(h):
    """x with fmix64(x) == h (the finalizer is a bijection: odd multipliers and xor-shifts)."""
    h = _unxorshift33(h)
    h = (h * pow(0xc4ceb9fe1a85ec53, -1, 2 ** 64)) & MASK
    h = _unxorshift33(h)
    h = (h * pow(0xff51afd7ed558ccd, -1, 2 ** 64)) & MASK
    return _unxorshift33(h)


def kmer_hashes(seq, k, seed=0):
    """h of every valid cyclic k-mer of seq, in the order of their starts."""
    seq = bytes(seq)
    n = len(seq)
    if n < k:
        return []
    fwd = seq.translate(_DIGITS).decode()
    rev = fwd[::-1].encode().translate(_COMPLEMENT).decode()       # the reverse complement, digit by digit ('x' stays)
    fwd2, rev2 = fwd + fwd, rev + rev
    out = []
    for p in range(n):
        w = fwd2[p:p + k]
        if "x" in w:
            continue
        q = (n - p - k) % n                                         # where the k-mer's reverse complement starts on the other strand
        f, r = int(w, 4), int(rev2[q:q + k], 4)
        out.append(fmix64(min(f, r) ^ seed))
    return out


def sketch(seq, k, log2_bins, seed=0):
    """(row, n_kmers) of one record: row a list of 1 << log2_bins integers."""
    row = [EMPTY] * (1 << log2_bins)
    hashes = kmer_hashes(seq, k, seed)
    for h in hashes:
        b = h >> (64 - log2_bins)
        if h < row[b]:
            row[b] = h
    return row, len(hashes)


def sketch_batch(seqs, k, log2_bins, seed=0):
    """(rows (n, bins) uint64, counts uint32) of a list of records."""
    rows = np.empty((len(seqs), 1 << log2_bins), dtype=np.uint64)
    counts = np.zeros(len(seqs), dtype=np.uint32)
    for i, s in enumerate(seqs):
        row, counts[i] = sketch(s, k, log2_bins, seed)
        rows[i] = np.array(row, dtype=np.uint64)
    return rows, counts


def compare(a, b):
    """(match, filled) of two rows, bin by bin."""
    match = filled = 0
    for x, y in zip(a, b):
        x, y = int(x), int(y)
        match += x == y and x != EMPTY
        filled += x != EMPTY or y != EMPTY
    return match, filled


def compare_pairs(rows_a, rows_b, pairs):
    """(match, filled, n_invalid) over a list of pairs; an invalid pair is (0, 0).  The same counts as compare(), as array
    expressions (test_sketch_cpu.py holds the two against each other)."""
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    match = np.zeros(len(pairs), dtype=np.uint32)
    filled = np.zeros(len(pairs), dtype=np.uint32)
    ok = (pairs[:, 0] < len(rows_a)) & (pairs[:, 1] < len(rows_b))
    idx = np.flatnonzero(ok)
    for at in range(0, len(idx), 4096):
        sel = idx[at:at + 4096]
        x, y = rows_a[pairs[sel, 0].astype(np.int64)], rows_b[pairs[sel, 1].astype(np.int64)]
        match[sel] = ((x == y) & (x != np.uint64(EMPTY))).sum(axis=1)
        filled[sel] = ((x != np.uint64(EMPTY)) | (y != np.uint64(EMPTY))).sum(axis=1)
    return match, filled, int((~ok).sum())


def revcomp(seq):
    return bytes(seq)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))
