"""The FASTA texts of the device parser's tests and their yardstick: the host packer circkit_fasta_parse (ckhost::parse_chunk),
called on the same text with the same flags.  Shared by tests/test_fasta_device_cpu.py (the CPU fiber program) and
tests/test_fasta_device_gpu.py (the device).

A text is left out under a flag pair only where the host routine does not answer deterministically: without first_chunk a
text that begins with '\\n' makes it read the byte in front of the text (its header search starts AT the record start)."""
import ctypes
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_examples")
FLAG_PAIRS = ((True, True), (True, False), (False, True), (False, False))
FORMAT_ERROR = "FASTA parse error: expected '>' at the start of the first record"


def deterministic(text, first, final):
    return first or not bytes(text).startswith(b"\n")


_cache = {}


def host(text, first=True, final=True):
    """circkit_fasta_parse on `text`: dict(error, records, consumed, offsets, data, head, raw) with head / raw as (R, 2) uint64
    arrays of (off, len); error = the message, with zero records.  Computed once per (text, flags) and shared: do not modify."""
    text = bytes(text)
    key = (text, bool(first), bool(final))
    if key in _cache:
        return _cache[key]
    import circkit_amd
    lib = circkit_amd.load_library()
    buf = ctypes.create_string_buffer(text, max(len(text), 1))
    h, consumed = ctypes.c_void_p(), ctypes.c_size_t(0)
    rc = lib.circkit_fasta_parse(ctypes.addressof(buf), len(text), int(first), int(final), ctypes.byref(h), ctypes.byref(consumed))
    try:
        if rc != 0:
            res = dict(error=lib.circkit_fasta_error(h).decode(), records=0, consumed=0, offsets=np.zeros(1, dtype=np.uint64),
                       data=np.zeros(0, dtype=np.uint8), head=np.zeros((0, 2), dtype=np.uint64), raw=np.zeros((0, 2), dtype=np.uint64))
        else:
            n = lib.circkit_fasta_n_records(h)
            offs = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_offsets(h), ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy()
            total = int(offs[-1])
            data = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_bytes(h), ctypes.POINTER(ctypes.c_uint8)), shape=(max(total, 1),)).copy()[:total]
            head, raw = np.zeros((n, 2), dtype=np.uint64), np.zeros((n, 2), dtype=np.uint64)
            ho, hl, ro, rl = (ctypes.c_size_t(0) for _ in range(4))
            for i in range(n):
                lib.circkit_fasta_record(h, i, ctypes.byref(ho), ctypes.byref(hl), ctypes.byref(ro), ctypes.byref(rl))
                head[i] = (ho.value, hl.value)
                raw[i] = (ro.value, rl.value)
            res = dict(error=None, records=n, consumed=consumed.value, offsets=offs, data=data, head=head, raw=raw)
    finally:
        if h:
            lib.circkit_fasta_free(h)
    _cache[key] = res
    return res


def same(got, exp, what=""):
    """Every count, offset, payload byte and span of a device result (the dict of tests/emu/fasta_emu.run, or the GPU test's)
    against the host's."""
    if exp["error"]:
        assert got["refused"] == 3 and got["records"] == 0 and got["bytes"] == 0, (what, got["refused"], got["records"])
        return
    assert got["refused"] == 0, (what, got["refused"])
    assert (got["records"], got["consumed"], got["bytes"]) == (exp["records"], exp["consumed"], len(exp["data"])), \
        (what, got["records"], got["consumed"], got["bytes"], exp["records"], exp["consumed"], len(exp["data"]))
    assert np.array_equal(got["offsets"], exp["offsets"]), what
    assert np.array_equal(got["data"], exp["data"]), what
    if got.get("head") is not None:
        assert np.array_equal(got["head"], exp["head"]), (what, got["head"][:4], exp["head"][:4])
    if got.get("raw") is not None:
        assert np.array_equal(got["raw"], exp["raw"]), (what, got["raw"][:4], exp["raw"][:4])


# ---- the fixed list ----------------------------------------------------------------------------------------------------------
# the corner table the device parser was specified with: (text, first_chunk, final_chunk); each runs under the other flag pairs as well
TABLE = [
    (b"", True, True), (b"\n\r\n", True, True), (b"\r>a\nAC\n", True, True), (b" >a\n", True, True), (b">abc", True, True),
    (b">abc\r\n", True, True), (b">a\n>b\nAC\n>c", True, True), (b">a>b\nAC>G\n>c\nT", True, True), (b">a\nAC\r>b\nGG\n", True, True),
    (b">a\nAC\n>b\nGG\n>c\nTT", True, False), (b">a\nACGT\nAC", True, False), (b">a\nAC\n>", True, False),
    (b"XYZ\nAC\n>b\nGG\n>c", False, False), (b"\n\n>a\nAC", True, False),
]

CORNERS = [
    b">a\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",                          # CRLF
    b">a\r\nACGT\r\n>b\r\nGG\r",                                   # ... and a lone \r at the end of the text
    b">a\nAC\r",
    b">a\r",
    b">a\n\nAC\n\n\nGT\n\n>b\n\n\n>c\nT\n\n",                      # blank lines inside and between records
    b"\n\n\r\n>a\nAC\n",
    b">a b c  d\nAC\n>x>y >z\nGT\n>\t tab\nA\n",                   # headers with spaces and '>'
    b">\nAC\n>\n>\n\n>e\n",                                        # empty headers, empty sequences
    b">\n", b">\r\n", b">", b">>", b">>>>>>>>", b">\n>\n>\n>",
    b">s\nacgtnACGTN\nuUtT\nRYKMSWBDHVN rykm\n.~-*\n a c\tg t \n",  # lower case, uU, IUPAC, .~, spaces, tabs
    b">hi\n" + bytes(range(0x80, 0x100)) + b"\n" + bytes(range(0, 0x80)).replace(b">", b"") + b"\n",     # every byte value
    b">no newline at all ACGT",
    b"ACGT no start, no newline",
    b">a\nAC\n>b",
    b">a\nAC\n>b\n",
    b">a\nAC\r\n>b\r\nG>G\r>\r\n",
    b"\r\r\n\r>a\n>b\n",
    b">a\n>",
    b"A", b"\r", b"\n", b" ",
]


def golden_texts():
    paths = sorted(glob.glob(os.path.join(GOLDEN, "*", "in.fasta"))) + [os.path.join(GOLDEN, "test.fasta")]
    return [(os.path.relpath(p, GOLDEN), open(p, "rb").read()) for p in paths]


# ---- seeded random texts -----------------------------------------------------------------------------------------------------
def _alphabet():
    """Weighted toward '>', the line ends, the bases and their neighbours, with arbitrary bytes on top."""
    w = np.ones(256)
    w[ord(">")] = 40
    w[ord("\n")] = 60
    w[ord("\r")] = 25
    for ch in b"ACGTacgunN-. ":
        w[ch] = 30
    return w / w.sum()


def random_texts(seed, count, lo, hi):
    rng = np.random.default_rng(seed)
    p = _alphabet()
    out = []
    for k in range(count):
        n = int(rng.integers(lo, hi + 1))
        t = rng.choice(256, size=n, p=p).astype(np.uint8)
        if n and k % 3 == 0:            # a proper beginning, so that first_chunk accepts most of them
            t[0] = ord(">")
        if n > 400 and k % 2 == 0:      # long runs without an event: lines and headers longer than a tile
            a = int(rng.integers(0, n - 200))
            b = int(rng.integers(a, n))
            t[a:b] = rng.choice(np.frombuffer(b"ACGTacgtN ", dtype=np.uint8), size=b - a)
        out.append(t.tobytes())
    return out


def small_cases():
    """[(name, text, first, final)]: the fixed list and 300 random texts of 0..200 bytes, each under all four flag pairs."""
    texts = [("table%d" % k, t) for k, (t, _, _) in enumerate(TABLE)] + [("corner%d" % k, t) for k, t in enumerate(CORNERS)] + golden_texts() + \
        [("random%d" % k, t) for k, t in enumerate(random_texts(20261, 300, 0, 200))]
    return [(name, t, first, final) for name, t in texts for first, final in FLAG_PAIRS if deterministic(t, first, final)]


def large_cases():
    """40 random texts of 1..64 KiB under all four flag pairs."""
    texts = [("large%d" % k, t) for k, t in enumerate(random_texts(20262, 40, 1024, 65536))]
    return [(name, t, first, final) for name, t in texts for first, final in FLAG_PAIRS if deterministic(t, first, final)]


def records_text(rng, n_records, length, width=0, crlf=False):
    """n_records records of `length` bases, on one line each (width 0) or wrapped."""
    eol = b"\r\n" if crlf else b"\n"
    parts = []
    for i in range(n_records):
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=length).tobytes()
        parts.append(b">r%d some text" % i + eol)
        if width:
            parts.extend(seq[a:a + width] + eol for a in range(0, length, width))
        else:
            parts.append(seq + eol)
    return b"".join(parts)


def tile_edge_texts(T):
    """[(name, text, first, final)] of what sits on the seams of tiles of T bytes."""
    rng = np.random.default_rng(5)
    out = []
    for n in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1):
        t = records_text(rng, 2 * n // 100 + 2, 90, width=40)[:n]
        out.append(("length%d" % n, t))
    head = b">h\n"
    for at in (T, T - 1, 2 * T, 2 * T - 1):                                  # a record start at a tile's first / last byte
        body = head + b"A" * (at - len(head) - 1) + b"\n"
        out.append(("start_at%d" % at, body + b">next\nACGT\nGG\n>z\nT"))
    out.append(("header_2.5_tiles", b">" + b"h" * (5 * T // 2) + b"\r\nAC\nGT\n>b\nA\n"))
    out.append(("line_3_tiles", b">a\n" + b"ACGT" * (3 * T // 4) + b"\n>b\n" + b"acgu" * 10 + b"\n"))
    out.append(("dropped_tile", b">a\nAC" + b" \t\r\n" * (T // 2) + b"GT\n>b\n" + b"\n" * (T + 7) + b"T"))
    out.append(("header_tile_then_seq", b">" + b"x" * (2 * T) + b"\n" + b"N" * (2 * T + 3)))
    return [(name, t, f, l) for name, t in out for f, l in FLAG_PAIRS if deterministic(t, f, l)]
