"""Shared input sets for the parity tests (oracle vs emulator on CPU, oracle vs HIP on the GPU)."""
import random

import numpy as np


def pack(seqs):
    lens = [len(s) for s in seqs]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    data = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    return data, offs


def rand_seq(rng, n, alpha=b"ACGT"):
    return bytes(rng.choice(alpha) for _ in range(n))


def revcomp_acgt(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def adversarial(seed=11):
    """SURVEY.md 8d adversarial set + boundary lengths of the packed-word machinery."""
    rng = random.Random(seed)
    S = [b"", b"A", b"T", b"AC", b"CA", b"ATGCA", b"AAA", b"ATT", b"TAA", b"banana", b"TGCA", b"GCAT",
         b"AATCAATTTCCTCCATCACCTAGTTTATGTAGAAACGCTGCTA", b"TCCTCCATCACCTAGTTTATGTAGAAACGCTGCTAAATCAATT"]
    for n in (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 255, 256, 257, 1000, 1008, 1023,
              1024, 1025, 1040, 2047, 2048, 2049, 3000):
        S.append(b"A" * n)                                   # all-A
        S.append(b"A" * (n - 1) + b"T")                      # A...AT
        S.append(b"T" + b"A" * (n - 1))                      # TA...A
        S.append(b"T" * n)                                   # max key everywhere
        S.append(rand_seq(rng, n))
        S.append(rand_seq(rng, n, b"ACGTN"))                 # 4-bit mode
        S.append(rand_seq(rng, n, b"ACGTN-"))
        S.append(rand_seq(rng, n, b"AC"))                    # low complexity
        if n <= 300:
            S.append(bytes(rng.randint(0x20, 0x7E) for _ in range(n)))   # arbitrary ASCII: 8-bit mode
            S.append(rand_seq(rng, n, b"ACGTRYKMacgtn"))
    for p in (1, 2, 3, 5, 7, 16, 17, 48, 50, 64, 100):        # period-p repeats, p | n and p does not divide n
        unit = rand_seq(rng, p)
        for reps in (2, 3, 10, 21):
            S.append(unit * reps)
            S.append((unit * reps)[:-1] if len(unit * reps) > 1 else unit)
            t = bytearray(unit * reps)
            t[-1] = ord("T") if t[-1] != ord("T") else ord("A")          # one mismatch at the end
            S.append(bytes(t))
            S.append(unit * reps + b"N")
    for n in (50, 64, 200, 1000):                            # reverse palindromes: fwd == rc
        h = rand_seq(rng, n // 2)
        S.append(h + revcomp_acgt(h))
    for _ in range(20):                                      # rotations / strand flips of one record
        base = rand_seq(rng, rng.randint(48, 400))
        k = rng.randrange(len(base))
        S.append(base[k:] + base[:k])
        S.append(revcomp_acgt(base))
    # poly-A runs inside random sequence, tandem repeats embedded in unique flanks
    for _ in range(20):
        a = rand_seq(rng, rng.randint(30, 500))
        S.append(a + b"A" * rng.randint(17, 80) + rand_seq(rng, rng.randint(30, 500)) + b"A" * rng.randint(17, 80))
        u = rand_seq(rng, rng.randint(1, 20))
        S.append(a + u * rng.randint(3, 30) + rand_seq(rng, 40) + u * rng.randint(3, 30))
    return S


def random_mixed(seed, count, lo, hi, alpha=b"ACGT"):
    rng = random.Random(seed)
    return [rand_seq(rng, rng.randint(lo, hi), alpha) for _ in range(count)]


def expected(O, s):
    """(canonical bytes, strand, reference-visible index) from the oracle."""
    l = O.lmsr(s)
    rc = O.lmsr(O.revcomp(l))
    fwd = l < rc
    idx = O.lmsr_index(s) if fwd else O.lmsr_index(O.revcomp(l))
    return (l if fwd else rc), (0 if fwd else 1), idx


# ---- one record set per kernel path (tests/test_gpu_outputs.py) -----------------------------------------------------
# Each kind aims at one route through launch_canon; KIND_MODES is what circkit_ctx_last_batch_mode must report for it, so that a
# kind cannot quietly stop covering its route.  Small on purpose (a few MB each): every kind runs under 15 output sets x 3.
def _np_seq(rng, n, alpha=b"ACGT", p=None):
    return bytes(np.frombuffer(alpha, dtype=np.uint8)[rng.choice(len(alpha), size=n, p=p)])


def _sprinkle(rng, s, frac, chars=b"N-"):
    b = bytearray(s)
    for p in rng.integers(0, len(b), size=max(1, int(len(b) * frac))):
        b[int(p)] = chars[int(rng.integers(0, len(chars)))]
    return bytes(b)


def k1kb(seed=1):
    """300..1008 ACGT, most of them longer than 800 (not MODE_SHORT): the one-record-per-wave builds, the group hash fused
    into them"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(801, 1009, size=1500), rng.integers(300, 801, size=1000)])
    return [_np_seq(rng, int(n)) for n in rng.permutation(lens)]


def kshort(seed=2):
    """mostly 48..600 ACGT, plus 1..47 and XXH3's short / long edge (239, 240, 241): MODE_SHORT pair builds, rescue pass"""
    rng = np.random.default_rng(seed)
    S = [_np_seq(rng, int(n)) for n in rng.integers(48, 601, size=3000)]
    S += [_np_seq(rng, int(n)) for n in rng.integers(1, 48, size=200)]
    S += [_np_seq(rng, n) for n in (239, 240, 241) for _ in range(40)]
    return [S[i] for i in rng.permutation(len(S))]


def kalpha(seed=3):
    """1 kb with 1..5 % N and '-': MODE_ALPHA builds, the 4-bit register routine"""
    rng = np.random.default_rng(seed)
    S = [_sprinkle(rng, _np_seq(rng, int(n)), float(rng.uniform(0.01, 0.05))) for n in rng.integers(900, 1009, size=1500)]
    return S + [_np_seq(rng, 1000) for _ in range(100)]


def ktwo(seed=4):
    """1009..2032 ACGT: the ROWS = 2 builds"""
    rng = np.random.default_rng(seed)
    S = [_np_seq(rng, int(n)) for n in rng.integers(1009, 2033, size=1500)]
    return S + [_np_seq(rng, n) for n in (1009, 1024, 1025, 2031, 2032)]


def kmixed(seed=5):
    """log-uniform 200 b .. 20 kb, plain and with 1 % N: the mixed-length kernel and LDS tiers A / B / C"""
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(200), np.log(20000), size=700)).astype(int)
    return [_sprinkle(rng, _np_seq(rng, int(n)), 0.01, b"N") if i % 2 else _np_seq(rng, int(n)) for i, n in enumerate(lens)]


def klong(seed=6):
    """20..80 kb (team mode), N inside the winning window (4-bit team), and records beyond the on-chip tiers (> 640 kb of
    ACGT, > 100 kb of 0x21..0x7e): the global-scratch stages"""
    rng = np.random.default_rng(seed)
    S = [_np_seq(rng, int(n)) for n in rng.integers(20000, 80001, size=24)]
    for n in (21000, 33000, 47000):                    # the minimal window (a run of A) with an N inside; the reverse strand too
        body = _np_seq(rng, n, b"CGT")
        run = b"A" * 14 + b"N" + b"A" * 3
        S.append(body[:n // 3] + run + body[n // 3:])
        S.append(revcomp_acgt(body[:n // 2] + b"A" * 20 + body[n // 2:]).replace(b"G", b"N", 3))
    S += [_sprinkle(rng, _np_seq(rng, 30000), 0.01, b"N-") for _ in range(3)]
    S.append(_np_seq(rng, 700_000))
    S.append(_np_seq(rng, 120_000, bytes(range(0x21, 0x7F))))
    return [S[i] for i in rng.permutation(len(S))]


def kodd(seed=7):
    """every byte value, lower-case IUPAC, "", repeats, reverse-complement palindromes, rotations of one record: where the
    index convention (smallest minimal rotation; the count from the forward minimum on the reverse strand) matters"""
    rng = np.random.default_rng(seed)
    S = adversarial(seed)
    S += [bytes(range(256)), bytes(range(255, -1, -1)), bytes(rng.integers(0, 256, size=3000).astype(np.uint8)),
          bytes(rng.integers(0, 256, size=700).astype(np.uint8)), _np_seq(rng, 1500, b"acgtnrykmswbdhv"), b"", b"", b"A" * 4000,
          b"AC" * 1200, _np_seq(rng, 37) * 60, (_np_seq(rng, 37) * 30)[:-5]]
    for n in (100, 1000, 2000, 6000):
        h = _np_seq(rng, n // 2)
        S.append(h + revcomp_acgt(h))
    base = _np_seq(rng, 1500)
    for k in rng.integers(0, 1500, size=10):
        S += [base[int(k):] + base[:int(k)], revcomp_acgt(base[int(k):] + base[:int(k)])]
    return S


KINDS = {"k1kb": k1kb, "kshort": kshort, "kalpha": kalpha, "ktwo": ktwo, "kmixed": kmixed, "klong": klong, "kodd": kodd}
# the mode every kind must report (circkit_ctx_last_batch_mode); ktwo is mode 3 when the hash is wanted without index / strand /
# lmsr (launch_canon: the mixed-length kernels fuse XXH3 for two-word records); kodd: whatever it reports, 1..3
KIND_MODES = {"k1kb": 1, "kshort": 1, "kalpha": 1, "ktwo": 2, "kmixed": 3, "klong": 3, "kodd": None}


def kind_mode(kind, want_hash, want_index, want_strand, lmsr=False):
    if kind == "ktwo" and want_hash and not (want_index or want_strand or lmsr):
        return 3
    return KIND_MODES[kind]
