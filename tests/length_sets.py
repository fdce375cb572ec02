"""Record sets whose variable is the record's LENGTH, shared by the emulator tests (CPU) and the device tests (GPU).

Every build of the canonicalize kernels computes its lane constants from the record's length, from n mod 16 and from where the
record sits in its 16-byte chunk; launch_canon chooses among a dozen builds by the batch's mode and the outputs asked for.  This
module holds
  * the crafted sets of tests/test_emu_kernel.py (same seeds, same RNG calls in the same order as when they lived there),
  * one "every length" sweep per route through launch_canon (ROUTES), in two orders, and
  * expected_mode(): batch_mode_of restated from the rules as DESIGN.md states them, so that a set cannot quietly stop reaching
    its route.
Pure Python + numpy: no GPU, no emulator."""
import random

import numpy as np

from tests import seqsets


# ---- the crafted sets (tests/test_emu_kernel.py; tests/test_canon_lengths_gpu.py runs them on the device) --------------------
def sprinkle(rng, s, frac, ch=ord("N")):
    b = bytearray(s)
    for i in range(len(b)):
        if rng.random() < frac:
            b[i] = ch
    return bytes(b)


def mixed_batch(seed, with_n):
    rng = random.Random(seed)
    seqs = seqsets.random_mixed(seed + 1, 40, 48, 1008) + seqsets.random_mixed(seed + 2, 30, 1009, 9000) + \
        seqsets.random_mixed(seed + 3, 6, 1, 47) + [b"", b"ACGT" * 400, b"A" * 3000]
    for n in (1100, 2500, 4097):                                          # long reverse-complement palindromes, rotations, repeats
        h = seqsets.rand_seq(rng, n // 2)
        seqs.append(h + seqsets.revcomp_acgt(h))
        base = seqsets.rand_seq(rng, n)
        k = rng.randrange(n)
        seqs += [base, base[k:] + base[:k], seqsets.revcomp_acgt(base)]
        u = seqsets.rand_seq(rng, 37)
        seqs.append(seqsets.rand_seq(rng, 600) + u * 40 + seqsets.rand_seq(rng, 500))
        seqs.append(seqsets.rand_seq(rng, 700) + b"A" * 40 + seqsets.rand_seq(rng, 900) + b"A" * 40)        # the minimal key twice
    if with_n:
        seqs = [sprinkle(rng, s, 0.01) if i % 5 else s for i, s in enumerate(seqs)]
        seqs += [sprinkle(rng, seqsets.rand_seq(rng, 3000), 0.02, ord("-")), sprinkle(rng, seqsets.rand_seq(rng, 500), 0.3)]
    rng.shuffle(seqs)
    return seqs


def register_routine_with_n_mask(staged):
    """48..80, 990..1008 and the powers of two with a few N each, then planted A-runs with an N / G / T / C behind them"""
    rng = np.random.default_rng(1700 + staged)
    comp = bytes.maketrans(b"ACGTN", b"TGCAN")
    seqs = []
    for L in list(range(48, 81)) + list(range(990, 1009)) + [127, 128, 129, 255, 256, 257, 511, 512, 513]:
        s = bytearray(seqsets.random_mixed(1701 + L, 1, L, L)[0])
        for p in rng.integers(0, L, size=max(1, L // 100)):
            s[int(p)] = ord("N")
        seqs.append(bytes(s))
    for case in range(150):
        L = int(rng.integers(200, 1009))
        bg = bytearray(rng.choice(list(b"CGT"), size=L, p=[0.2, 0.4, 0.4]).astype(np.uint8).tobytes())
        run = int(rng.integers(2, 15))
        for sp in sorted(rng.choice(np.arange(10, L - 30, 25), size=int(rng.integers(1, 4)), replace=False)):
            motif = b"A" * run + bytes(rng.choice(list(b"NGTCN"), size=1).astype(np.uint8)) + bytes(rng.choice(list(b"ACGTN"), size=5, p=[.23, .23, .23, .23, .08]).astype(np.uint8))
            if rng.random() < 0.5:
                motif = motif.translate(comp)[::-1]
            bg[sp:sp + len(motif)] = motif
        seqs.append(bytes(bg))
    return seqs


def mixed_prefix_rule_and_extension_edges():
    rng = random.Random(77)
    seqs = []
    for k in range(48):
        n = rng.randint(1100, 2600)
        s = bytearray(seqsets.rand_seq(rng, n, b"CGT"))
        pos = rng.choice([0, 1, 7, n - 1, n - 9, n - 16, n - 17, n // 2])
        for i in range(18):
            s[(pos + i) % n] = ord("A")                                   # the minimal key, wrapping around the end for some
        if k % 3 == 0:
            s[(pos + rng.randint(3, 22)) % n] = ord("N")                 # ...with an N inside or just behind it
        if k % 3 == 1:
            s = bytearray(seqsets.revcomp_acgt(bytes(s).replace(b"N", b"A")))   # the reverse strand wins
            s[rng.randrange(n)] = ord("N")
        seqs.append(bytes(s) + seqsets.rand_seq(rng, k % 16, b"G"))       # shifts the next record's alignment
    return seqs


def mixed_tied_minimal_key():
    rng = random.Random(91)
    seqs = []
    for k in range(40):
        n_runs = rng.randint(2, 5)
        run = b"A" * (16 if k % 5 else rng.randint(17, 18))
        parts = []
        for _ in range(n_runs):
            parts.append(run + seqsets.rand_seq(rng, rng.randint(200, 900), b"CGT"))
        s = b"".join(parts)
        if k % 4 == 0:
            s = seqsets.revcomp_acgt(s)                                   # the reverse strand wins
        seqs.append(s + seqsets.rand_seq(rng, k % 16, b"G"))
    seqs += [seqsets.rand_seq(rng, 700, b"CGT") * 3, b"ACGT" * 500]       # periods: stage A's
    return seqs


def mixed_winner_seen_twice_by_one_lane(with_n):
    rng = random.Random(123)
    seqs = []
    for n in list(range(1010, 1075, 3)) + list(range(2040, 2100, 5)) + [3073, 3080, 4104, 5131]:
        s = bytearray(seqsets.rand_seq(rng, n, b"CGT"))
        pos = rng.choice([0, 1, 2, 9, 15, 16, 17, n - 1, n - 2, n - 15, n - 16, n - 17, n - 31])
        for i in range(16):
            s[(pos + i) % n] = ord("A")
        if with_n:
            s[(pos + 40) % n] = ord("N")
        seqs.append((seqsets.revcomp_acgt(bytes(s).replace(b"N", b"C")) if n % 2 else bytes(s)) + seqsets.rand_seq(rng, n % 16, b"G"))
    return seqs


def mixed_minimal_key_inside_a_palindrome():
    rng = random.Random(321)
    seqs = []
    for k in range(30):
        half = b"A" * rng.randint(6, 9) + seqsets.rand_seq(rng, rng.randint(1, 4), b"ACGT")
        pal = half + seqsets.revcomp_acgt(half)                          # self reverse-complementary, starts with the A run
        body = seqsets.rand_seq(rng, rng.randint(1100, 4000), b"CGT")
        s = body[:len(body) // 3] + pal + body[len(body) // 3:]
        seqs.append(s + seqsets.rand_seq(rng, k % 16, b"G"))
    for n in (1200, 2600):
        h = seqsets.rand_seq(rng, n // 2)
        seqs.append(h + seqsets.revcomp_acgt(h))
    return seqs


def mixed_n_inside_the_minimal_window():
    rng = random.Random(2025)
    seqs = [sprinkle(rng, seqsets.rand_seq(rng, rng.randint(1009, 2600)), rng.choice([0.01, 0.03, 0.08])) for _ in range(40)]
    seqs += [sprinkle(rng, seqsets.rand_seq(rng, rng.randint(1009, 2200), b"AC"), 0.02) for _ in range(6)]
    for k in range(40):
        n = rng.randint(1100, 2400)
        s = bytearray(seqsets.rand_seq(rng, n, b"CGT"))
        pos, pos2 = rng.randrange(n), rng.randrange(n)
        for i in range(rng.randint(8, 16)):
            s[(pos + i) % n] = ord("A")
        s[(pos + k % 13) % n] = ord("N")
        for i in range(rng.randint(5, 10)):
            s[(pos2 + i) % n] = ord("A")
        s = bytes(s)
        seqs.append(s if k % 2 else seqsets.revcomp_acgt(s.replace(b"N", b"X")).replace(b"X", b"N"))
    return seqs


def mixed_with_fused_xxh3(with_n):
    """mixed_batch plus lengths around every XXH3 block and stripe boundary"""
    rng = random.Random(515)
    seqs = mixed_batch(5150, with_n)
    for n in (241, 255, 256, 257, 1009, 1023, 1024, 1025, 1087, 1088, 1089, 2047, 2048, 2049, 2111, 2112, 2113, 3072, 3073, 4095, 4096, 4097, 5121):
        seqs.append(seqsets.rand_seq(rng, n))
        seqs.append(seqsets.revcomp_acgt(seqsets.rand_seq(rng, n, b"CGT") + b"A" * 17))
    rng.shuffle(seqs)
    return seqs


def pair_two_records_per_wave(staged):
    """every combination of a record the pair routine takes with a partner it does not, lengths on and off the 16-symbol grid"""
    rng = random.Random(4100 + staged)
    R = lambda n, al=b"ACGT": seqsets.rand_seq(rng, n, al)
    pal = R(40)
    pal = pal + seqsets.revcomp_acgt(pal)                                             # its own reverse complement
    odd = [b"", R(7), R(47), R(1009), R(1500), R(3000), R(500)[:250] + b"N" + R(249), R(300) + b"-" + R(300), b"ACGT" * 200, b"A" * 777,
           (R(31) * 40)[:900], pal * 8, b"T" * 48, R(100, b"AC"), bytes(range(0x30, 0x7B)) * 5]
    good = [R(n) for n in (48, 49, 63, 64, 65, 240, 241, 255, 256, 257, 511, 512, 513, 527, 528, 529, 992, 1000, 1007, 1008)]
    seqs = []
    for g in good:
        o = rng.choice(odd)
        seqs += [g, o] if rng.random() < 0.5 else [o, g]
    for _ in range(60):
        seqs += [R(rng.randint(48, 1008)), R(rng.randint(48, 1008))]
    seqs += [R(1000) for _ in range(40)]                                               # (equal lengths: the lane constants are reused)
    seqs += [R(rng.choice([48, 64, 1008])) for _ in range(16)]
    return seqs


def pair_every_length():
    """every length 48..1008 once in either half of a wave, next to a partner of another length"""
    rng = random.Random(5150)
    lens = list(range(48, 1009))
    rng.shuffle(lens)
    seqs = []
    for i, n in enumerate(lens):
        a, b = seqsets.rand_seq(rng, n), seqsets.rand_seq(rng, rng.randint(48, 1008))
        seqs += [a, b] if i % 2 else [b, a]
    # (`[...] * 0` adds nothing: its one 500-symbol draw is kept so that the RNG sequence, and with it the filler, stays what it was)
    seqs += [seqsets.rand_seq(rng, 500)] * 0 + [seqsets.rand_seq(rng, 700) for _ in range(16)]     # (the last group is never staged)
    return seqs


def hash_only_view_set():
    seqs = seqsets.random_mixed(7001, 40, 48, 1008) + seqsets.random_mixed(7002, 30, 1, 260) + seqsets.random_mixed(7003, 12, 1009, 2500) + \
        seqsets.random_mixed(7004, 20, 30, 900, b"ACGTN") + seqsets.random_mixed(7005, 8, 10, 400, b"-ACGNT") + \
        seqsets.random_mixed(7006, 6, 1, 300, bytes(range(0x21, 0x7F))) + seqsets.adversarial()[:60] + [b"", b"ACGTRYKMacgtn" * 30]
    rng = np.random.default_rng(7007)
    return [seqs[i] for i in rng.permutation(len(seqs))]


# ---- batch_mode_of, restated ---------------------------------------------------------------------------------------------------
MODE_ALPHA, MODE_SHORT = 4, 8
ONE_WORD_MAX, TWO_WORD_MAX, SHORT_MAX = 1008, 2032, 800
LENGTH_SAMPLE_MAX, CONTENT_SAMPLES = 1 << 17, 4096


def content_samples(data, offs):
    """(bad, sampled): of up to 4096 evenly spaced records, how many hold a byte outside ACGT among their first 1008"""
    n = len(offs) - 1
    if n == 0:
        return 0, 0
    nc = min(n, CONTENT_SAMPLES)
    step = n // nc
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGT")] = True
    bad = 0
    for k in range(nc):
        a, b = int(offs[k * step]), int(offs[k * step + 1])
        if b - a >= 16:                                 # (the count kernel reads 16-byte chunks: shorter records are never looked at)
            bad += not ok[data[a:min(b, a + ONE_WORD_MAX)]].all()
    return bad, nc


def mode_counts(lengths, data, offs):
    """what the mode is decided from: records, long ones (> 2032), two-word ones (1009..2032), short ones (<= 800), content
    samples with a byte outside ACGT, content samples"""
    lengths = np.asarray(lengths, dtype=np.int64)
    n = len(lengths)
    assert n <= LENGTH_SAMPLE_MAX                       # every record is a length sample
    bad, sampled = content_samples(data, offs)
    return dict(n=n, lng=int((lengths > TWO_WORD_MAX).sum()), two=int(((lengths > ONE_WORD_MAX) & (lengths <= TWO_WORD_MAX)).sum()),
                short=int((lengths <= SHORT_MAX).sum()), bad=bad, sampled=sampled)


def expected_mode(lengths, data, offs, want_hash, aux):
    """The mode the device must report (bits 0..1: 1 one-word streaming builds, 2 two-word build, 3 mixed-length kernels; 4:
    MODE_ALPHA; 8: MODE_SHORT) for a batch whose outputs are `want_hash` and `aux` (index, strand or lmsr asked for)."""
    return mode_of_counts(mode_counts(lengths, data, offs), want_hash, aux)


def mode_of_counts(c, want_hash, aux):
    """expected_mode's rule, from mode_counts' counts"""
    m = 3 if c["lng"] and c["lng"] * 8 >= c["n"] else 2 if c["two"] and c["two"] * 4 >= c["n"] else 1
    alpha = MODE_ALPHA if c["bad"] and c["bad"] * 16 >= c["sampled"] else 0
    if m == 2 and (alpha or (want_hash and not aux)):
        m = 3
    short = MODE_SHORT if m == 1 and not alpha and c["short"] * 2 >= c["n"] else 0
    return m | alpha | short


# ---- one sweep per route ---------------------------------------------------------------------------------------------------------
def _acgt(rng, n):
    return seqsets._np_seq(rng, n)


def _with_n(rng, s):
    """max(1, n // 100) N at random positions"""
    if not s:
        return s
    b = bytearray(s)
    for p in rng.integers(0, len(b), size=max(1, len(b) // 100)):
        b[int(p)] = ord("N")
    return bytes(b)


MIXED_LENGTHS = sorted(set(range(48, 3137)) | {1024 * k + d for k in range(1, 21) for d in (-17, -16, -1, 0, 1, 16, 17)})
SHORT_CLASSES = list(range(0, 48))                  # with the ranges below: every length 0..260 of XXH3's short-input classes

# route: probe lengths, extra lengths below the range (XXH3's short classes), N in every record, the filler (count, length), the
# canonicalize output sets and the lmsr output sets to run, the mode & 3 every one of them must report, the emulator geometry
# (`staged`) per output set for the path evidence, and the seed.
ROUTES = {
    "stream_bytes": dict(lengths=range(48, 1009), short=[], n=False, filler=(2100, 1000), outs=["b"], lmsr=[], mode={"b": 1}, staged={"b": 1}, seed=101),
    "pair_bytes": dict(lengths=range(48, 1009), short=[], n=False, filler=(32, 500), outs=["b"], lmsr=[], mode={"b": 1}, staged={"b": 14}, seed=102),
    "pair_hash": dict(lengths=range(48, 1009), short=SHORT_CLASSES, n=False, filler=(32, 700), outs=["bh", "h"], lmsr=[], mode={"bh": 1, "h": 1},
                      staged={"bh": 15, "h": 15}, seed=103),
    "stream_n": dict(lengths=range(48, 1009), short=SHORT_CLASSES, n=True, filler=(64, 1000), outs=["b", "bh", "h"], lmsr=[],
                     mode={"b": 1, "bh": 1, "h": 1}, staged={"b": 16, "bh": 13, "h": 13}, seed=104),
    "aux_one_word": dict(lengths=range(48, 1009), short=[], n=False, filler=(32, 1000), outs=["bis"], lmsr=["bi"], mode={"bis": 1, "lmsr bi": 1},
                         staged={}, seed=105),
    "two_word": dict(lengths=range(1009, 2033), short=[], n=False, filler=(32, 1500), outs=["b", "bis"], lmsr=["bi"],
                     mode={"b": 2, "bis": 2, "lmsr bi": 2}, staged={"b": 17}, seed=106),
    "two_word_hash": dict(lengths=range(1009, 2033), short=[], n=False, filler=(32, 1500), outs=["bh", "h"], lmsr=[], mode={"bh": 3, "h": 3},
                          staged={}, seed=107),
    "mixed": dict(lengths=MIXED_LENGTHS, short=SHORT_CLASSES, n=False, filler=(0, 1000), outs=["b", "bh", "h"], lmsr=[],
                  mode={"b": 3, "bh": 3, "h": 3}, staged={}, seed=108),
    "mixed_n": dict(lengths=MIXED_LENGTHS, short=SHORT_CLASSES, n=True, filler=(0, 1000), outs=["b", "bh", "h"], lmsr=[],
                    mode={"b": 3, "bh": 3, "h": 3}, staged={}, seed=109),
}
ORDERS = ("as_built", "shifted")

_SWEEPS = {}


def sweep(route, order="as_built"):
    """(records, probe flags): the route's probes -- one record of every length, shuffled, random over the route's alphabet --
    followed by the filler that fixes the mode (the streaming kernels never stage a batch's last group, so it is filler).
    `shifted`: one more filler record in front, which moves every probe to the other half-wave of a pair build, to the
    neighbouring wave of the others, and changes its alignment in its chunk.  probe flags: True for the records of the route's
    own range (not the short classes, not the filler)."""
    if route not in _SWEEPS:
        r = ROUTES[route]
        rng = np.random.default_rng(r["seed"])
        lens = list(r["lengths"]) + list(r["short"])
        lens = [lens[i] for i in rng.permutation(len(lens))]
        lo = min(r["lengths"])
        probes = [_acgt(rng, n) for n in lens]
        fill = [_acgt(rng, r["filler"][1]) for _ in range(r["filler"][0] + 1)]
        if r["n"]:
            probes = [_with_n(rng, s) for s in probes]
            fill = [_with_n(rng, s) for s in fill]
        _SWEEPS[route] = (probes, [n >= lo for n in lens], fill)
    probes, flags, fill = _SWEEPS[route]
    if order == "as_built":
        return probes + fill[1:], flags + [False] * (len(fill) - 1)
    assert order == "shifted"
    return fill[:1] + probes + fill[1:], [False] + flags + [False] * (len(fill) - 1)


# ---- the crafted sets as device batches: filler of the routes' kinds where a set alone would not give the mode it aims at -------
def _long_filler(seed, seqs):
    """mode 3: long records are at least 1/8 of the batch -- here a quarter and more"""
    rng = np.random.default_rng(seed)
    return seqs + [_acgt(rng, 3000) for _ in range(len(seqs) // 3 + 1)]


def _tail_filler(seed, seqs, count, length, n=False):
    rng = np.random.default_rng(seed)
    fill = [_acgt(rng, length) for _ in range(count)]
    return seqs + ([_with_n(rng, s) for s in fill] if n else fill)


# name: (builder, mode its emulator test aims at -- bits 0..1, MODE_ALPHA, and for the bytes-only call MODE_SHORT; None: whatever
# expected_mode says --, output sets)
def crafted_mode_matches(aim, mode, outs):
    """does expected_mode's answer for a call with `outs` carry what the set aims at: bits 0..1 and MODE_ALPHA (which pick the build
    among the alphabets' twins), and MODE_SHORT where it picks one (bytes only: the pair build)"""
    bits = 3 | MODE_ALPHA | (MODE_SHORT if outs == "b" else 0)
    return aim is None or (mode & bits) == (aim & bits)


CRAFTED = {
    "n_mask_1": (lambda: _tail_filler(201, register_routine_with_n_mask(1), 64, 1000, True), 1 | MODE_ALPHA, ["b", "bh", "h"]),
    "n_mask_3": (lambda: _tail_filler(202, register_routine_with_n_mask(3), 64, 1000, True), 1 | MODE_ALPHA, ["b", "bh", "h"]),
    "pair_two_records_14": (lambda: _tail_filler(203, pair_two_records_per_wave(14), 32, 700), 1 | MODE_SHORT, ["b", "bh", "h"]),
    "pair_two_records_15": (lambda: _tail_filler(204, pair_two_records_per_wave(15), 32, 700), 1 | MODE_SHORT, ["b", "bh", "h"]),
    "pair_every_length": (pair_every_length, 1 | MODE_SHORT, ["b", "bh", "h"]),
    "mixed_batch": (lambda: _long_filler(205, mixed_batch(4000, False)), 3, ["b", "bh", "h"]),
    "mixed_batch_n": (lambda: _long_filler(206, mixed_batch(4000, True)), 3 | MODE_ALPHA, ["b", "bh", "h"]),
    "mixed_prefix_rule": (lambda: _long_filler(207, mixed_prefix_rule_and_extension_edges()), 3 | MODE_ALPHA, ["b", "bh", "h"]),
    "mixed_tied_key": (lambda: _long_filler(208, mixed_tied_minimal_key()), 3, ["b", "bh", "h"]),
    "mixed_seen_twice": (lambda: _long_filler(209, mixed_winner_seen_twice_by_one_lane(False)), 3, ["b", "bh", "h"]),
    "mixed_seen_twice_n": (lambda: _long_filler(210, mixed_winner_seen_twice_by_one_lane(True)), 3 | MODE_ALPHA, ["b", "bh", "h"]),
    "mixed_palindrome": (lambda: _long_filler(211, mixed_minimal_key_inside_a_palindrome()), 3, ["b", "bh", "h"]),
    "mixed_n_in_window": (lambda: _long_filler(212, mixed_n_inside_the_minimal_window()), 3 | MODE_ALPHA, ["b", "bh", "h"]),
    "mixed_fused_xxh3": (lambda: _long_filler(213, mixed_with_fused_xxh3(False)), 3, ["b", "bh", "h"]),
    "mixed_fused_xxh3_n": (lambda: _long_filler(214, mixed_with_fused_xxh3(True)), 3 | MODE_ALPHA, ["b", "bh", "h"]),
    "hash_only_views": (hash_only_view_set, None, ["h", "bh"]),
}
