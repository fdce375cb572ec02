"""Existing input sets placed round byte 2^32 of a payload buffer (TEST INFRASTRUCTURE ONLY, pure numpy): where the absolute
offsets go, what lies in the alias region a position truncated to 32 bits would read, and the list of sets that
tests/test_high_base_gpu.py runs.  tests/test_high_base_cpu.py checks the conditions on these inputs without a GPU.

The device entry points take 64-bit CSR offsets and mix them with 32-bit lengths and in-record positions; a set placed here has
records below the line, one record across it (or starting exactly on it) and records above it, so that a 32-bit slip in a payload
position reads the decoy instead of the record."""
import functools

import numpy as np

LINE = 2 ** 32
HALF = 4 << 20                                   # the payload lies in [LINE - HALF, LINE + HALF)
BIG = LINE + 2 * HALF                            # bytes of the device buffer
MODES = ("middle", "boundary")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_NEXT = np.arange(256, dtype=np.uint8)           # another ACGT byte: A -> C -> G -> T -> A, anything else stays
for _a, _b in zip(b"ACGT", b"CGTA"):
    _NEXT[_a] = _b


def place(offsets, j, mode, at=0):
    """The absolute offsets `offsets + lead`.  "middle": record j straddles the line, offsets[j] + lead < LINE < offsets[j+1] +
    lead, the line as near its middle as possible.  "boundary": offsets[j] + at + lead == LINE (at = 0: record j starts exactly on
    the line, low word 0; at > 0 puts the line on position `at` of record j).  The payload must fit [LINE - HALF, LINE + HALF)."""
    o = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    a, b = int(o[j]), int(o[j + 1])
    if mode == "middle":
        assert at == 0 and b - a >= 2, "a record of fewer than 2 bytes has no byte pair for the line to fall between"
        lead = LINE - (a + b) // 2
    elif mode == "boundary":
        assert 0 <= at <= b - a
        lead = LINE - a - at
    else:
        raise ValueError(mode)
    assert LINE - HALF <= int(o[0]) + lead and int(o[-1]) + lead <= LINE + HALF, "the set does not fit the window round the line"
    return (o + lead).astype(np.uint64)


def decoy(seed, n):
    """n seeded random ACGT bytes for the alias region [0, n) of the big buffer."""
    return _ACGT[np.random.default_rng(seed).integers(0, 4, size=int(n))]


def differing(dec, data, absolute):
    """`dec` with every byte that a payload position p >= LINE aliases (dec[p - LINE]) made different from the payload's byte
    there: where the two random bytes agree, the decoy takes the next letter of ACGT.  A one-byte record differs from a random ACGT
    decoy with probability 3/4 only, and the sets hold hundreds of them; after this every record above the line, of any length
    but 0, reads a wrong answer from the alias, byte for byte."""
    dec = np.array(dec, dtype=np.uint8, copy=True)
    p0, p1 = int(absolute[0]), int(absolute[-1])
    assert p1 - p0 == len(data)
    if p1 > LINE:
        lo = max(p0, LINE)
        pay = np.asarray(data, dtype=np.uint8)[lo - p0:]
        q = dec[lo - LINE:p1 - LINE]
        dec[lo - LINE:p1 - LINE] = np.where(q == pay, _NEXT[q], q)
    return dec


def inner_longest(offsets, least=2):
    """The longest record that has a non-empty record on either side of it (the first of equals): with it on the line, a record
    lies wholly below the line and one wholly above.  None when no such record has `least` bytes."""
    n = np.diff(np.asarray(offsets, dtype=np.uint64).astype(np.int64))
    filled = np.flatnonzero(n > 0)
    if len(filled) < 3:
        return None
    lo, hi = int(filled[0]), int(filled[-1])
    j = lo + 1 + int(np.argmax(n[lo + 1:hi]))
    return j if n[j] >= least else None


def conditions(data, offsets, j, mode, at=0, dec=None):
    """What tests/test_high_base_cpu.py asserts of one placed set; returns the absolute offsets."""
    absolute = place(offsets, j, mode, at)
    o = absolute.astype(np.int64)
    n = np.diff(o)
    if mode == "middle":
        assert o[j] < LINE < o[j + 1] and abs((LINE - o[j]) - (o[j + 1] - LINE)) <= 1
    else:
        assert o[j] + at == LINE and (at or (int(o[j]) & 0xFFFFFFFF) == 0)
    assert ((o[1:] <= LINE) & (n > 0)).any(), "no record wholly below the line"
    assert ((o[:-1] >= LINE) & (n > 0)).any(), "no record wholly above the line"
    assert LINE - HALF <= o[0] and o[-1] <= LINE + HALF
    dec = differing(decoy(1, HALF) if dec is None else dec, data, absolute)
    data = np.asarray(data, dtype=np.uint8)
    for i in np.flatnonzero((o[:-1] >= LINE) & (n > 0)):
        rec = data[o[i] - o[0]:o[i + 1] - o[0]]
        assert (dec[o[i] - LINE:o[i + 1] - LINE] != rec).all(), "record %d equals its alias somewhere" % i
    return absolute


def pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(bytes(s) for s in seqs) + b"\0", dtype=np.uint8)[:int(offs[-1])].copy(), offs


# ---- the sets of Part A ---------------------------------------------------------------------------------------------------------
SKETCH_PARAMS = ((21, 8), (32, 8), (4, 4))


@functools.lru_cache(maxsize=None)
def sketch_records(kind, k):
    """(records, j): sketch_sets.length_records(k) or symbol_records(k) with one record of 3 * SKETCH_SEG + 500 symbols in their
    middle.  In "middle" mode the line falls inside that record's second span."""
    from tests import sketch_sets as S
    seg = S.constants()["SKETCH_SEG"]
    recs = list(S.length_records(k) if kind == "lengths" else [s for _, s in S.symbol_records(k)])
    j = len(recs) // 2
    recs.insert(j, S.with_symbol(S.random_acgt(np.random.default_rng(1000 + k), 3 * seg + 500), [seg - 1, 2 * seg]))
    return tuple(recs), j, seg


@functools.lru_cache(maxsize=None)
def mono_records():
    """(records, j): mono_sets.adversarial(), j = the first 2 x 1100 dimer (one substitution in its first copy)."""
    from tests import mono_sets as S
    seqs = S.adversarial()
    j = next(i for i, s in enumerate(seqs) if len(s) == 2200)
    return tuple(seqs), j


def framed(case):
    """A monomer compact case between a head and a tail record of 3 bytes each, both without an end index: every record of the
    case proper then has a non-empty record on either side, whatever its own neighbours are."""
    name, data, offs, ends, full_len, flt = case
    rng = np.random.default_rng(len(data) + 31 * len(offs))
    head, tail = decoy(int(rng.integers(1 << 30)), 3), decoy(int(rng.integers(1 << 30)), 3)
    offs = np.asarray(offs, dtype=np.uint64)
    offs2 = np.concatenate([[0], offs + np.uint64(3), [offs[-1] + np.uint64(6)]]).astype(np.uint64)
    none = np.array([0xFFFFFFFF], dtype=np.uint32)
    full2 = None if full_len is None else np.concatenate([[3], np.asarray(full_len, dtype=np.uint64), [3]]).astype(np.uint64)
    return (name, np.concatenate([head, data, tail]), offs2, np.concatenate([none, np.asarray(ends, dtype=np.uint32), none]), full2, flt)


@functools.lru_cache(maxsize=None)
def monomers_cases():
    """[(case, j or None)]: monomers_sets.emulator_sets(tile) and misalignment_set(), framed.  j = the longest record of the case
    proper; None when that has fewer than 2 bytes (no byte pair for the line to fall between): such a case runs on the boundary
    alone, with the line at the start of the tail record."""
    from tests import monomers_sets as MS
    out = []
    for c in MS.emulator_sets(MS.constants()["TILE_BYTES"]) + [MS.misalignment_set()]:
        f = framed(c)
        out.append((f, inner_longest(f[2])))
    return tuple(out)


NO_MIDDLE = ("only empty records, keep_all", "payload of 1 bytes", "payload of 1 bytes in single bytes", "payload of 5 bytes in single bytes",
             "payload of 15 bytes in single bytes", "payload of 16 bytes in single bytes")


UNIQ_COUNT, UNIQ_P, UNIQ_BASES = 1000, (0.3, 0.9), (0, 2 ** 32 + 12345)


@functools.lru_cache(maxsize=None)
def uniq_cases():
    """[(name, data, offsets, first_seen, base, j)]: 1000 records of 0..40 bytes, first_seen as tests/test_uniq_compact_gpu.py crafts
    it (kept, an earlier record of the batch, a record of an earlier batch, ~0) with keep probability 0.3 and 0.9, base 0 and
    2^32 + 12345 (d_dup_first then carries global indices above 2^32)."""
    from tests import monomers_sets as MS
    from tests.test_uniq_compact_gpu import crafted
    out = []
    for p in UNIQ_P:
        for base in UNIQ_BASES:
            rng = np.random.default_rng(UNIQ_COUNT + int(10 * p) + (base & 1))
            data, offs = MS.batch(rng, rng.integers(0, 41, size=UNIQ_COUNT))
            out.append(("uniq p=%g base=%d" % (p, base), data, offs, crafted(rng, UNIQ_COUNT, p, base), base, inner_longest(offs)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def windows_cases():
    from tests import windows_sets as S
    return tuple(S.all_cases())


@functools.lru_cache(maxsize=None)
def translate_cases():
    from tests import translate_sets as S
    return tuple(S.all_cases())


@functools.lru_cache(maxsize=None)
def fasta_write_cases():
    """The cases of grid_cases() and label_cases() that take their bodies from a batch (the others have no d_body to place)."""
    from tests import fasta_write_sets as S
    return tuple(c for c in S.grid_cases() + S.label_cases() if c.body is not None)


def body_of(c):
    """(payload, offsets from 0) of a FASTA write case's body batch: the bytes in front of offsets[0] belong to no record."""
    o = c.offsets.astype(np.int64)
    return c.body[o[0]:o[-1]], (o - o[0]).astype(np.uint64)


CANON_CRAFTED = ("mixed_fused_xxh3", "pair_two_records_15")


@functools.lru_cache(maxsize=None)
def canon_sets():
    """{name: records}: one record of every length 0..2100 in a seeded order (every tenth with an N, every 37th arbitrary bytes),
    and the two crafted sets of tests/length_sets.py."""
    from tests import length_sets as LS
    rng = np.random.default_rng(2100)
    seqs = []
    for n in rng.permutation(2101).tolist():
        s = bytearray(_ACGT[rng.integers(0, 4, size=n)].tobytes())
        if n and n % 10 == 3:
            s[int(rng.integers(0, n))] = ord("N")
        if n and n % 37 == 5:
            s[int(rng.integers(0, n))] = int(rng.integers(0x21, 0x7F))
        seqs.append(bytes(s))
    out = {"every_length": tuple(seqs)}
    for name in CANON_CRAFTED:
        out[name] = tuple(LS.CRAFTED[name][0]())
    return out


def sets():
    """Every placement of Part A: (name, data, offsets from 0, j, mode, at)."""
    out = []
    for kind in ("lengths", "symbols"):
        for k, _ in SKETCH_PARAMS:
            recs, j, seg = sketch_records(kind, k)
            data, offs = pack(recs)
            out += [("sketch %s k%d" % (kind, k), data, offs, j, "middle", 0), ("sketch %s k%d" % (kind, k), data, offs, j, "boundary", 0),
                    ("sketch %s k%d span" % (kind, k), data, offs, j, "boundary", seg)]
    recs, j = mono_records()
    data, offs = pack(recs)
    out += [("monomerize", data, offs, j, m, 0) for m in MODES]
    for (name, data, offs, _, _, _), j in monomers_cases():
        if j is not None:
            out.append(("monomers " + name, data, offs, j, "middle", 0))
        out.append(("monomers " + name, data, offs, len(offs) - 2 if j is None else j, "boundary", 0))
    for name, data, offs, _, _, j in uniq_cases():
        out += [(name, data, offs, j, m, 0) for m in MODES]
    for what, cases in (("windows", windows_cases()), ("translate", translate_cases())):
        for c in cases:
            out += [("%s %s" % (what, c[0]), c[1], c[2], inner_longest(c[2]), m, 0) for m in MODES]
    for c in fasta_write_cases():
        data, offs = body_of(c)
        out += [("fasta write " + c.name, data, offs, inner_longest(offs), m, 0) for m in MODES]
    for name, recs in canon_sets().items():
        data, offs = pack(recs)
        out += [("canon " + name, data, offs, inner_longest(offs), m, 0) for m in MODES]
    return out


# ---- the tiled FASTA text of tests/test_past_4gib_gpu.py -------------------------------------------------------------------------
def block_of(pad):
    """A few whole records, messy as tests/fasta_sets.py's texts are: multi-line sequences, lower case, \\r\\n, a blank line, a U,
    IUPAC letters, a '>' inside a header; `pad` lengthens the first header."""
    return (b">r0 " + b"x" * pad + b" first\n" + b"ACGTTGCAAC" * 8 + b"\n" + b"GGGTTTAAAC" * 8 + b"\nACG\n"
            b">r1 lower case, crlf\r\nacgtnacgtt\r\nTTGACCA\r\n"
            b">r2 a blank line inside\nACGTAC\n\nGTTGCA\n"
            b">r3 rna >and iupac\nACGUUGCAuuRYKM\nNNNN-ACGT\n"
            b">r4\nA\n")


def where_line_falls(block):
    """'sequence', 'header' or 'record start': what byte 2^32 of the tiled text is."""
    at = LINE % len(block)
    if block[at:at + 1] == b">" and (at == 0 or block[at - 1:at] == b"\n"):
        return "record start"
    start = block.rfind(b"\n>", 0, at + 1) + 1 if at else 0
    eol = block.find(b"\n", start)
    if at <= eol:
        return "header" if start < at < eol - 1 else "other"
    return "sequence" if block[at:at + 1] in b"ACGTUacgtunRYKMN-" and block[at - 1:at] not in b"\n\r" and block[at + 1:at + 2] not in b"\n\r" else "other"


def block_for(where):
    """The first block (shortest pad) that puts byte 2^32 of the tiled text where asked."""
    for pad in range(0, 40000):
        b = block_of(pad)
        if where_line_falls(b) == where and (where != "record start" or LINE % len(b) != 0):
            return b
    raise AssertionError(where)
