"""Record sets and settings shared by the monomerize tests (emulator, GPU, driver).  Everything is seeded."""
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXAMPLES = os.path.join(HERE, "golden", "ref_examples")
FIXTURES = {"min_overlap": dict(min_overlap=81), "min_overlap_percent_0.51": dict(min_overlap_percent=0.51),
            "min_overlap_percent_1.0": dict(min_overlap_percent=1.0), "min_overlap_percent_1.5": dict(min_overlap_percent=1.5)}

# (seed_len, cut-off) pairs every adversarial record runs under, plain and sensitive
DISTS = (0, 1, 5, 2 ** 63)
IDENTITIES = (0.0, 0.5, 0.9, 0.94, 0.95, 1.0)


def settings(seeds=(1, 5, 10, 63)):
    out = []
    for k in seeds:
        for d in DISTS:
            out.append(dict(seed_len=k, max_mismatch=d))
        for ident in IDENTITIES:
            out.append(dict(seed_len=k, min_identity=ident))
    return [dict(s, sensitive=sv) for s in out for sv in (False, True)]


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    data = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:int(offs[-1])].copy()
    return data, offs


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def periodic(rng, n, p, alpha=b"ACGT", subs=0):
    mon = rand_seq(rng, p, alpha)
    s = bytearray((mon * (n // p + 1))[:n])
    for _ in range(subs):
        if n:
            s[rng.randrange(n)] = rng.choice(alpha)
    return bytes(s)


def bump(b):
    """Another byte for a substitution (A -> C -> G -> T -> A, anything else -> A)."""
    return {65: 67, 67: 71, 71: 84, 84: 65}.get(b, 65)


def substituted(s, positions):
    s = bytearray(s)
    for p in positions:
        s[p] = bump(s[p])
    return bytes(s)


def every_length(rng, upto=300):
    """One record of every length 0..upto, periodic with a few substitutions so that some monomerize."""
    return [periodic(rng, n, rng.randint(1, max(1, n // 2 + 1)), subs=rng.randint(0, 2)) for n in range(upto + 1)]


def adversarial(seed=7, long_poly=3000):
    rng = random.Random(seed)
    out = [b"TGCCAATGCATGCCAATGC", b"", b"A", b"AC"]
    out += [b"A" * n for n in (2, 19, 20, 21, 126, 127, 128, 1000, 1024, 1025, long_poly)]
    for n, p in ((1000, 250), (1000, 333), (1000, 7), (2048, 1024), (2049, 1024), (2047, 1023), (3000, 1000), (3000, 999), (600, 200),
                 (600, 199), (126, 63), (127, 63), (128, 64)):
        out.append(periodic(rng, n, p))
        out.append(periodic(rng, n, p, subs=3))
    for alpha in (b"ACGTN-", b"AC", b"N-", bytes(range(256)), bytes(range(128, 256))):
        for n, p in ((700, 300), (64, 20), (1500, 700)):
            out.append(periodic(rng, n, p, alpha))
            out.append(periodic(rng, n, p, alpha, subs=2))
    # a dimer x.x of 2 * 1100: one substitution in the first copy at the first / last byte of the overlap and on both sides
    # of every 16-byte edge counted from either end (the count runs from the end, the sensitive one from the front), which
    # covers the 1024-byte step edges (1100 - 1024 = 76 from the front, 1024 from the front)
    L = 1100
    x = rand_seq(rng, L)
    edges = {0, L - 1, 1023, 1024, L - 1024, L - 1025}
    for e in range(16, L, 16):
        edges |= {e - 1, e, L - e - 1, L - e}
    for r in sorted(e for e in edges if 0 <= e < L):
        out.append(substituted(x, [r]) + x)
    out.append(x + substituted(x, [0]))
    out.append(x + substituted(x, [L - 1]))
    # the occurrence (plain: at r - k of x + x[:r]; sensitive: at len(x)) at the first and last position of a scan step
    for k in (1, 5, 10, 63):
        for p in (0, 15, 16, 1008, 1023, 1024, 1039, 1040, 2047, 2048):
            y = rand_seq(rng, 2600)
            out.append(y + y[:p + k])
    for ln in (1009, 1023, 1024, 1025, 1040, 2047, 2048, 2049):
        y = rand_seq(rng, ln)
        out.append(y + y[:200])
        out.append(y + substituted(y[:200], [100]))
    return out


def distinct_kmers(rng, n, k):
    """A random ACGT string of n symbols whose k-mers are all different."""
    while True:
        s = rand_seq(rng, n)
        if len({s[i:i + k] for i in range(n - k + 1)}) == n - k + 1:
            return s


def max_dist(ovl, identity):
    """lib/src/monomerize.rs:70-76 in f64."""
    import math
    return ovl - int(math.floor(float(ovl) * identity))


def identity_boundaries(seed=11, k=5):
    """[(record, identity, ovl, n_mismatches, accepted)]: dimers x'.x with an overlap of ovl symbols and exactly max_dist
    or max_dist + 1 substitutions outside the seed zone of the first copy.  x has no repeated k-mer, and the record is
    redrawn until the seed occurs in it twice only (in each copy's last k symbols), so the one candidate is the overlap ovl."""
    rng = random.Random(seed)
    out = []
    for ovl in (19, 20, 40, 100):
        for ident in IDENTITIES:
            md = max_dist(ovl, ident)
            for extra in (0, 1):
                nm = md + extra
                if nm > ovl - k:
                    continue                       # no room outside the seed zone (identity 0 and 0.5 on short overlaps)
                while True:
                    x = distinct_kmers(rng, ovl, k)
                    first = substituted(x, rng.sample(range(ovl - k), nm))
                    t, seed_ = first + x, x[-k:]
                    if [i for i in range(len(t) - k + 1) if t[i:i + k] == seed_] == [ovl - k, 2 * ovl - k]:
                        break
                out.append((first + x, ident, ovl, nm, extra == 0))
    return out


def rolling(seed, lengths, pmin=150, pmax=700, rate=0.01, chunk=50000):
    """Rolling-circle records: record i is a random ACGT monomer of pmin..pmax symbols repeated to lengths[i] symbols, every
    base then substituted by another with probability `rate`.  Returns (data, offsets)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    data = np.empty(int(offs[-1]), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for a in range(0, len(lengths), chunk):
        ln = lengths[a:a + chunk]
        m = len(ln)
        p = rng.integers(pmin, pmax + 1, size=m)
        mon = rng.integers(0, 4, size=(m, pmax), dtype=np.uint8)
        total = int(ln.sum())
        if (ln == ln[0]).all():                    # one length: a rectangle
            idx = (np.arange(int(ln[0]), dtype=np.int32)[None, :] % p[:, None].astype(np.int32))
            codes = np.take_along_axis(mon, idx, axis=1).reshape(-1)
        else:
            rec = np.repeat(np.arange(m, dtype=np.int64), ln)
            start = np.zeros(m, dtype=np.int64)
            start[1:] = np.cumsum(ln)[:-1]
            pos = np.arange(total, dtype=np.int64) - start[rec]
            codes = mon[rec, pos % p[rec]]
        hit = rng.random(total) < rate
        codes = (codes + hit * rng.integers(1, 4, size=total, dtype=np.uint8)) & 3
        data[int(offs[a]):int(offs[a]) + total] = lut[codes]
    return data, offs


def random_records(seed, lengths):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return lut[rng.integers(0, 4, size=int(offs[-1]), dtype=np.uint8)], offs


def extended_realistic():
    """nim_cated/realistic_input.fasta with every record extended by its first half: (fasta_text, n_records, originals)."""
    from oracle import oracle as O
    text = open(os.path.join(EXAMPLES, "nim_cated", "realistic_input.fasta"), "rb").read()
    recs = [(h, O.full_seq(r)) for h, r in O.read_fasta(text)]
    out = b"".join(b">" + h + b"\n" + s + s[:len(s) // 2] + b"\n" for h, s in recs)
    return out, len(recs), {h: s for h, s in recs}


def fasta_map(data):
    """id -> sequence (the reference's check_fasta compares these maps)."""
    from oracle import oracle as O
    return {O.record_id(h): O.full_seq(r) for h, r in O.read_fasta(data)}
