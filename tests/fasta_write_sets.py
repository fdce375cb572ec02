"""The cases of the device FASTA writer's tests and their yardstick: the Python join b">" + head + label + b"\\n" + body + b"\\n" per
record, with the validity rules of include/circkit.h restated.  Shared by tests/test_fasta_write_cpu.py (the CPU fiber program)
and tests/test_fasta_write_gpu.py (the device)."""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_examples")
WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])
EXACT = 2 ** 64 - 1
ALIAS_TEXT, ALIAS_BODY = 1, 2
# 0, and both sides of every power of ten a u32 reaches, and the largest
LABEL_STARTS = [0] + [v for e in range(1, 10) for v in (10 ** e - 1, 10 ** e)] + [2 ** 32 - 1]


class Case:
    """One write: the text with its head (and raw) spans, the map, the labels, the body batch, and where the buffers lie
    (place: text_shift, body_shift, out_shift, capacity, alias, alias_at)."""

    def __init__(self, name, text, head, raw=None, body=None, offsets=None, src=None, n_src=None, labels=None, n_out=None, **place):
        self.name, self.text = name, bytes(text)
        self.head = np.ascontiguousarray(head, dtype=np.uint64).reshape(-1, 2)
        self.raw = None if raw is None else np.ascontiguousarray(raw, dtype=np.uint64).reshape(-1, 2)
        self.body = None if body is None else np.ascontiguousarray(np.frombuffer(bytes(body), dtype=np.uint8))
        self.offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        self.src = None if src is None else np.ascontiguousarray(src, dtype=np.uint64)
        self.n_src = len(self.head) if self.src is None else len(self.src) if n_src is None else n_src
        self.labels = None if labels is None else np.ascontiguousarray(labels, dtype=WINDOW_DTYPE)
        assert (self.body is None) == (self.offsets is None) and (self.body is None) != (self.raw is None)
        self.n_out = n_out if n_out is not None else len(self.offsets) - 1 if self.offsets is not None else \
            len(self.labels) if self.labels is not None else self.n_src
        self.place = place

    def moved(self, name, **place):
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name, c.place = name, dict(self.place, **place)
        return c


def label_of(strand, start):
    return (b"_RC_ORF" if strand else b"_ORF") + str(int(start)).encode()


def expected(c):
    """([record k's bytes, b"" for an invalid record], invalid records): the join, and the rules of circkit_fasta_write_device."""
    n, out, bad = len(c.text), [], 0
    inside = lambda off, ln: not (off > n or ln > n - off)
    b0 = int(c.offsets[0]) if c.offsets is not None and c.n_out else 0
    b1 = int(c.offsets[c.n_out]) if c.offsets is not None and c.n_out else 0
    for k in range(c.n_out):
        rec = None
        i, label = k, b""
        ok = True
        if c.labels is not None:
            L = c.labels[k]
            ok = int(L["strand"]) <= 1 and int(L["reserved"]) == 0
            i = int(L["record"])
            if ok:
                label = label_of(int(L["strand"]), int(L["start"]))
        if ok and i < c.n_src:
            h = int(c.src[i]) if c.src is not None else i
            if h < len(c.head) and inside(int(c.head[h][0]), int(c.head[h][1])):
                head = c.text[int(c.head[h][0]):int(c.head[h][0]) + int(c.head[h][1])]
                if c.body is not None:
                    o0, o1 = int(c.offsets[k]), int(c.offsets[k + 1])
                    if b0 <= o0 <= o1 <= b1:
                        rec = b">" + head + label + b"\n" + c.body[o0:o1].tobytes() + b"\n"
                elif inside(int(c.raw[h][0]), int(c.raw[h][1])):
                    rec = b">" + head + label + b"\n" + c.text[int(c.raw[h][0]):int(c.raw[h][0]) + int(c.raw[h][1])] + b"\n"
        bad += rec is None
        out.append(rec or b"")
    return out, bad


def check(c, got, what=""):
    """got: (text | None, out_offsets, total, n_invalid, refused) of an accepted write, against the join."""
    recs, bad = expected(c)
    text, off, total, n_invalid, refused = got
    want = b"".join(recs)
    name = what or c.name
    assert refused == 0, (name, refused)
    assert (total, n_invalid) == (len(want), bad), (name, total, n_invalid, len(want), bad)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)), name
    assert bytes(text) == want, (name, next(k for k in range(min(len(text), len(want)) + 1) if bytes(text[k:k + 1]) != want[k:k + 1]))


# ---- building blocks -------------------------------------------------------------------------------------------------------
def letters(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=int(n))])


HEAD_ALPHABET = b"abcdefghijklmnopqrstuvwxyz0123456789 _|.:>"


def layout(heads, raws=None, junk=b""):
    """A text that holds the heads (and the raw sequences) as a FASTA file would, after `junk`: (text, head spans, raw spans)."""
    parts, at, hs, rs = [junk], len(junk), [], []
    for k, h in enumerate(heads):
        r = raws[k] if raws is not None else b""
        hs.append((at + 1, len(h)))
        rs.append((at + 2 + len(h), len(r)))
        rec = b">" + h + b"\n" + r + b"\n"
        parts.append(rec)
        at += len(rec)
    return b"".join(parts), np.array(hs, dtype=np.uint64).reshape(-1, 2), np.array(rs, dtype=np.uint64).reshape(-1, 2)


def pack(bodies, lead=b""):
    """A CSR batch behind `lead` bytes that belong to no record: (bytes, offsets with offsets[0] = len(lead))."""
    offs = np.zeros(len(bodies) + 1, dtype=np.uint64)
    offs[0] = len(lead)
    offs[1:] = len(lead) + np.cumsum([len(b) for b in bodies], dtype=np.int64) if len(bodies) else []
    return lead + b"".join(bodies), offs


def windows(rows):
    """[(record, start, strand[, reserved])] as WINDOW_DTYPE."""
    w = np.zeros(len(rows), dtype=WINDOW_DTYPE)
    for k, row in enumerate(rows):
        w[k] = (77 + k, row[0], row[1], row[2], row[3] if len(row) > 3 else 0)
    return w


# ---- the sets --------------------------------------------------------------------------------------------------------------
def grid_cases():
    """Head length x body length over 0..33 each (and eight 3-byte records in a row in front: five whole records in one granule),
    all in one batch, at each of the 16 output shifts; the text and body shifts sweep along.  Every fourth batch takes its bodies
    from the raw spans."""
    out = []
    for k in range(16):
        rng = np.random.default_rng(100 + k)
        sizes = [(0, 0)] * 8 + [(h, b) for h in range(34) for b in range(34)]
        heads = [letters(rng, h, HEAD_ALPHABET) for h, _ in sizes]
        bodies = [letters(rng, b, b"ACGTN-acgt\n\r") for _, b in sizes]
        place = dict(out_shift=k, text_shift=(5 * k + 3) % 16, body_shift=(11 * k + 7) % 16)
        if k % 4 == 3:
            text, hs, rs = layout(heads, bodies)
            out.append(Case("grid%d_raw" % k, text, hs, raw=rs, **place))
        else:
            text, hs, _ = layout(heads)
            body, offs = pack(bodies, lead=b"#" * (k % 5))
            out.append(Case("grid%d" % k, text, hs, body=body, offsets=offs, **place))
    return out


def long_cases(T):
    """A head and a body each longer than a tile of T output bytes; one record over three tiles."""
    rng = np.random.default_rng(7)
    heads = [b"a", letters(rng, T + 37, HEAD_ALPHABET), b"", letters(rng, 11, HEAD_ALPHABET), b"z"]
    bodies = [b"ACGT", letters(rng, T + 5), b"G", letters(rng, 3 * T + 11), b""]
    text, hs, rs = layout(heads, bodies)
    body, offs = pack(bodies)
    return [Case("long_body", text, hs, body=body, offsets=offs, out_shift=3, text_shift=9, body_shift=14),
            Case("long_raw", text, hs, raw=rs, out_shift=12, text_shift=1)]


def seam_cases(T):
    """Totals of T - 1, T, T + 1, 2T - 1, 2T + 1 bytes."""
    rng = np.random.default_rng(8)
    out = []
    for j, total in enumerate((T - 1, T, T + 1, 2 * T - 1, 2 * T + 1)):
        n = total // 96
        heads = [letters(rng, 5, HEAD_ALPHABET) for _ in range(n)]
        bodies = [letters(rng, 88) for _ in range(n - 1)] + [letters(rng, total - 96 * (n - 1) - 8)]
        text, hs, _ = layout(heads)
        body, offs = pack(bodies)
        c = Case("total%d" % total, text, hs, body=body, offsets=offs, out_shift=(3 * j) % 16, body_shift=j)
        assert sum(len(r) for r in expected(c)[0]) == total
        out.append(c)
    return out


def label_cases():
    """Every digit count on both strands; one header shared by many outputs."""
    rng = np.random.default_rng(9)
    heads = [b"plasmid_7 some description", b"x", b""]
    text, hs, _ = layout(heads, junk=b"junk\n")
    rows = [(k % 3 if k % 5 == 0 else 0, s, strand) for strand in (0, 1) for k, s in enumerate(LABEL_STARTS)]
    bodies = [letters(rng, int(n)) for n in rng.integers(0, 41, size=len(rows))]
    body, offs = pack(bodies)
    out = [Case("labels", text, hs, body=body, offsets=offs, labels=windows(rows), out_shift=5, text_shift=2),
           Case("labels_shift", text, hs, body=body, offsets=offs, labels=windows(rows[::-1]), out_shift=10, body_shift=3)]
    # the labels through a map, and with raw bodies: every output of a record repeats its raw sequence
    text2, hs2, rs2 = layout([b"r0", b"r1 d", b"r2"], [b"ACGT\nAC", b"", b"GG\r\nT"])
    out.append(Case("labels_map_raw", text2, hs2, raw=rs2, src=[2, 0], labels=windows([(0, 12, 1), (1, 3, 0), (1, 4000000000, 1), (0, 0, 0)]), out_shift=15))
    return out


def map_cases():
    """The kept-record map: identity, a permutation, repeats, a map shorter than the spans."""
    rng = np.random.default_rng(10)
    heads = [letters(rng, int(n), HEAD_ALPHABET) for n in rng.integers(0, 30, size=40)]
    raws = [letters(rng, int(n), b"ACGT\n") for n in rng.integers(0, 50, size=40)]
    text, hs, rs = layout(heads, raws)
    maps = dict(identity=np.arange(40), permutation=rng.permutation(40), repeats=rng.integers(0, 40, size=55), subset=np.sort(rng.permutation(40)[:17]))
    out = []
    for j, (name, m) in enumerate(maps.items()):
        bodies = [letters(rng, int(n)) for n in rng.integers(0, 60, size=len(m))]
        body, offs = pack(bodies, lead=b"!" * j)
        out.append(Case("map_" + name, text, hs, body=body, offsets=offs, src=m, out_shift=j, text_shift=2 * j + 1, body_shift=15 - j))
        out.append(Case("map_%s_raw" % name, text, hs, raw=rs, src=m, out_shift=8 + j, text_shift=j))
    return out


def invalid_cases():
    """Each kind of invalid record among valid neighbours, whose bytes must still be right."""
    rng = np.random.default_rng(11)
    heads = [letters(rng, int(n), HEAD_ALPHABET) for n in (4, 0, 9, 17, 3, 6)]
    raws = [letters(rng, int(n), b"ACGT\n") for n in (20, 5, 0, 33, 8, 2)]
    text, hs, rs = layout(heads, raws)
    n = len(text)
    bodies = [letters(rng, int(k)) for k in (7, 0, 19, 40, 3, 11)]
    body, offs = pack(bodies)
    out = []

    def both(name, head=hs, raw=rs, **kw):
        out.append(Case(name, text, head, body=body, offsets=offs, out_shift=len(out) % 16, **kw))
        if "labels" not in kw or len(kw["labels"]) == 6:
            out.append(Case(name + "_raw", text, head, raw=raw, out_shift=(len(out) + 5) % 16, **{k: v for k, v in kw.items() if k != "n_out"}))

    both("record_is_n_src", labels=windows([(0, 1, 0), (6, 2, 0), (2, 3, 1), (5, 4, 0), (6, 5, 1), (1, 6, 0)]))
    both("record_is_n_src_mapped", src=[3, 1, 4], labels=windows([(0, 1, 0), (3, 2, 0), (2, 3, 1), (1, 4, 0), (2 ** 32 - 1, 5, 1), (1, 6, 0)]))
    out.append(Case("more_outputs_than_records", text, hs, body=body, offsets=offs, src=[5, 4, 3, 2], out_shift=6))
    both("header_is_n_heads", src=[0, 6, 2, 2 ** 64 - 1, 4, 5])
    for name, span in (("one_past_the_text", (n - 3, 4)), ("off_past_the_text", (n + 1, 0)), ("wraps", (2 ** 64 - 1, 2)), ("len_wraps", (5, 2 ** 64 - 3)),
                       ("both_huge", (2 ** 63, 2 ** 63))):
        h2, r2 = hs.copy(), rs.copy()
        h2[2], r2[4] = span, span
        both("head_" + name, head=h2)
        out.append(Case("raw_" + name, text, hs, raw=r2, out_shift=len(out) % 16))
    h2 = hs.copy()
    h2[3] = (n, 0)                                                            # an empty span AT the end of the text is valid
    both("head_empty_at_the_end", head=h2)
    both("strand_2", labels=windows([(0, 1, 0), (1, 2, 2), (2, 3, 1), (3, 4, 2 ** 32 - 1), (4, 5, 1), (5, 6, 0)]))
    both("reserved_1", labels=windows([(0, 1, 0, 1), (1, 2, 0), (2, 3, 1, 2 ** 31), (3, 4, 0), (4, 5, 1), (5, 6, 0, 1)]))
    # a body range that decreases, and ranges that leave the payload [offsets[0], offsets[n_out])
    o2 = offs.copy()
    o2[2], o2[3] = o2[3], o2[2]
    out.append(Case("body_decreases", text, hs, body=body, offsets=o2, out_shift=4))
    o3 = offs.copy()
    o3[3] = o3[6] + 5
    out.append(Case("body_beyond_the_payload", text, hs, body=body + b"?" * 8, offsets=o3, out_shift=13))
    assert all(0 < expected(c)[1] < c.n_out for c in out if c.name != "head_empty_at_the_end" and c.name != "head_empty_at_the_end_raw")
    return out


def raw_cases():
    """Raw bodies: interior line ends of both kinds, and empty ones."""
    heads = [b"lf", b"crlf", b"empty", b"one", b"blank lines"]
    raws = [b"ACGT\nACGT\nAC", b"ACGT\r\nAC\r\nG", b"", b"A", b"AC\n\n\nGT\r\n\r\nA"]
    text, hs, rs = layout(heads, raws)
    return [Case("raw_bodies", text, hs, raw=rs, out_shift=7, text_shift=5), Case("raw_bodies_twice", text, hs, raw=rs, src=[1, 1, 2, 4, 0, 2, 3], out_shift=1)]


def _small(rng, count=30):
    heads = [letters(rng, int(n), HEAD_ALPHABET) for n in rng.integers(0, 25, size=count)]
    bodies = [letters(rng, int(n)) for n in rng.integers(0, 90, size=count)]
    text, hs, _ = layout(heads)
    return text, hs, bodies


def capacity_cases():
    """[(case, accepted)]: capacities of exactly the total, one less and 0; no records at all; a total that does not fit 64 bits."""
    text, hs, bodies = _small(np.random.default_rng(12))
    body, offs = pack(bodies)
    c = Case("capacity", text, hs, body=body, offsets=offs, out_shift=9)
    total = sum(len(r) for r in expected(c)[0])
    out = [(c.moved("capacity_exact", capacity=total), True), (c.moved("capacity_one_less", capacity=total - 1), False),
           (c.moved("capacity_0", capacity=0), False), (c.moved("capacity_more", capacity=total + 100), True)]
    empty_body, empty_offs = pack([])
    out.append((Case("no_records", text, hs, body=empty_body, offsets=empty_offs, src=np.zeros(0, dtype=np.uint64), capacity=0), True))
    out.append((Case("no_records_with_room", text, hs, body=empty_body, offsets=empty_offs, src=np.zeros(0, dtype=np.uint64), capacity=10, out_shift=3), True))
    huge = Case("total_beyond_64_bits", text, hs[:2], body=b"", offsets=[0, 2 ** 63, 2 ** 64 - 2], capacity=100)
    out.append((huge, False))
    return out


def overlap_cases():
    """[(case, accepted)]: an output that shares one byte with the text or with the body payload is refused, one that ends where
    they begin or begins where they end is accepted (the bytes in front of the payload, offsets[0] of them, belong to no record)."""
    text, hs, bodies = _small(np.random.default_rng(13), 12)
    lead = b"%" * 2000
    body, offs = pack(bodies, lead=lead)
    c = Case("overlap", text, hs, body=body, offsets=offs)
    total = sum(len(r) for r in expected(c)[0])
    assert total < len(lead)
    out = []
    for name, alias, span in (("text", ALIAS_TEXT, len(text)), ("body", ALIAS_BODY, len(body) - len(lead))):
        for at, ok in ((span - 1, False), (span // 2, False), (1 - total, False), (span, True), (-total, True)):
            out.append((c.moved("overlap_%s_at_%d" % (name, at), alias=alias, alias_at=at), ok))
    return out


def accepted_cases(T):
    return grid_cases() + long_cases(T) + seam_cases(T) + label_cases() + map_cases() + invalid_cases() + raw_cases()


# ---- whole files -----------------------------------------------------------------------------------------------------------
def golden_inputs():
    """{name: text} of the reference's own fixtures."""
    out = {os.path.basename(os.path.dirname(p)): open(p, "rb").read() for p in sorted(glob.glob(os.path.join(GOLDEN, "*", "in.fasta")))}
    out["realistic_input"] = open(os.path.join(GOLDEN, "nim_cated", "realistic_input.fasta"), "rb").read()
    return out


NOT_FOR_WINDOWS = ("repeated", "rna_input")      # normalize(raw) != full_seq(raw) there: canonicalize / uniq only
