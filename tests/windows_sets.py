"""Crafted batches and window lists for the windows gather, shared by its CPU fiber test and its GPU test (TEST INFRASTRUCTURE
ONLY).  A case is (name, data, offsets, windows, placement keywords); everything is seeded."""
import os
import re

import numpy as np

from tests.windows_ref import WINDOW_DTYPE, windows as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
RECORD_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 33, 100, 1000]
# what a record may hold: the table, not arithmetic on ACGT, has to complement these
ALPHABET = b"ACGT" * 6 + b"N-acgtnRYKMSWBDHVrykmswbdhv" + bytes([0, 1, 0x7F, 0x80, 0xFE, 0xFF, ord("U"), ord("u"), ord("."), ord("\n")])
WRAP = 2 ** 32 - 1


def constants():
    """The named constants of the windows gather: its geometry (window_gather.h) and the scan's (circkit_windows.hip)."""
    src = open(os.path.join(CSRC, "window_gather.h")).read() + open(os.path.join(CSRC, "circkit_windows.hip")).read()
    c = {}
    for name in ("GATHER_WAVES", "GATHER_STEPS", "WSCAN_WG", "WSCAN_ITEMS"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, name
        c[name] = int(m.group(1))
    c["TILE_BYTES"] = 64 * 16 * c["GATHER_STEPS"] * c["GATHER_WAVES"]
    c["WSCAN_TILE"] = c["WSCAN_WG"] * c["WSCAN_ITEMS"]
    c["WSCAN_CHUNK"] = c["WSCAN_WG"] * c["WSCAN_TILE"]         # windows per round of the single-workgroup second level
    return c


def batch(rng, lengths=RECORD_LENGTHS):
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    data = np.frombuffer(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), size=int(offs[-1]))]
    return data, offs


def grid(lengths, window_lengths=None, starts=None):
    """Every (record, window length, start, strand) of the issue's list, as rows for windows_ref.windows."""
    rows = []
    for r, n in enumerate(lengths):
        ls = window_lengths(n) if window_lengths else [0, 1, 15, 16, 17, n - 1, n, n + 1, 2 * n, 4 * n + 5]
        ss = starts(n) if starts else [0, 1, n - 1, n, n + 7, WRAP]
        for length in ls:
            for start in ss:
                if length < 0 or start < 0:
                    continue                              # n - 1 of an empty record
                rows += [(length, r, start, 0), (length, r, start, 1)]
    return rows


def invalid_rows(n_records):
    return [(5, n_records, 0, 0), (5, 1, 0, 2), (5, 2, 0, 0, 1), (2 ** 64 - 1, WRAP, WRAP, WRAP, WRAP)]


def main_case(rng):
    """The full grid over every record; the same record named by many consecutive windows; records in descending order; invalid
    windows between valid ones."""
    data, offs = batch(rng)
    nr = len(RECORD_LENGTHS)
    rows = grid(RECORD_LENGTHS)
    rows += [(3 + k % 5, 9, 7 * k, k & 1) for k in range(200)]                             # record 9 (100 symbols), 200 times in a row
    rows += [(1, 1, k, 0) for k in range(70)]                                             # 70 one-byte windows on the one-symbol record
    rows += [(RECORD_LENGTHS[r] + 2, r, 1, r & 1) for r in range(nr - 1, -1, -1)]          # descending records
    bad = invalid_rows(nr)
    mixed = []
    for k, row in enumerate(grid(RECORD_LENGTHS[:8], lambda n: [n, 17], lambda n: [n + 7])):
        mixed.append(row)
        if k % 3 == 0:
            mixed.append(bad[(k // 3) % len(bad)])
    return ("grid", data, offs, W(rows + mixed), {})


def shift_cases(rng):
    """A reduced set at every payload shift and every output shift mod 16: 16 passes, each shift once on either side."""
    lengths = [0, 1, 3, 16, 17, 33, 100]
    data, offs = batch(rng, lengths)
    rows = grid(lengths, lambda n: [1, 16, 17, n + 1, 2 * n], lambda n: [0, n - 1, n + 7]) + invalid_rows(len(lengths))[:2]
    wins = W(rows)
    return [("shift %d" % s, data, offs, wins, dict(in_shift=s, out_shift=(7 * s + 3) % 16, lead=s % 5)) for s in range(16)]


def boundary_cases(rng, c):
    """Window counts on both sides of a scan tile; total bytes and window counts on both sides of a gather tile; one window that
    spans several tiles, on either strand."""
    data, offs = batch(rng)
    nr = len(RECORD_LENGTHS)
    out = []
    for count in (c["WSCAN_TILE"] - 1, c["WSCAN_TILE"], c["WSCAN_TILE"] + 1, 2 * c["WSCAN_TILE"] + 1):
        w = np.zeros(count, dtype=WINDOW_DTYPE)
        w["length"] = rng.integers(0, 10, size=count)
        w["record"] = rng.integers(0, nr + 1, size=count)                                # (record nr: invalid)
        w["start"] = rng.integers(0, 2 ** 32, size=count)
        w["strand"] = rng.integers(0, 2, size=count)
        out.append(("scan count %d" % count, data, offs, w, dict(out_shift=count % 16)))
    per = c["TILE_BYTES"] // 16
    for count, last in ((per - 1, 16), (per, 15), (per, 16), (per, 17), (per + 1, 16)):
        rows = [(16, 4 + k % 7, 3 * k, k & 1) for k in range(count - 1)] + [(last, 10, 990, 1)]
        out.append(("tile: %d windows, the last of %d" % (count, last), data, offs, W(rows), {}))
    big = 2 * c["TILE_BYTES"] + 1234
    out.append(("a window across tiles", data, offs, W([(3, 3, 1, 0), (big, 10, 999, 0), (1, 1, 0, 1), (big, 8, 5, 1), (2, 2, 0, 0)]),
                dict(in_shift=9, out_shift=6, lead=2)))
    return out


def all_cases(c=None):
    c = c or constants()
    rng = np.random.default_rng(2025)
    return [main_case(rng)] + shift_cases(rng) + boundary_cases(rng, c)


def orf_records(seed=7, count=60, lo=2, hi=3000):
    """Normalized upper-case records for the ORF sequences: random ACGT, frames without a stop, multi-lap ORFs on records whose
    length is no multiple of 3, N and '-'."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [bytes(acgt[rng.integers(0, 4, size=int(n))]) for n in np.exp(rng.uniform(np.log(lo), np.log(hi), size=count)).astype(int)]
    seqs += [b"ATG" + b"C" * 997, b"CCAT" + b"G" * 500, b"ATG" + b"GCA" * 33 + b"G", b"ATG" + b"GCA" * 33 + b"GC", b"ATGAAA" * 40 + b"A",
             b"CAT" + b"TGC" * 50 + b"TT", b"ATGNNN-TAA" * 20, b"ATG" + b"N" * 200 + b"TAA", b"ATGATGTAG" * 12, b"TTACAT" * 30 + b"C", b"AT", b"TA"]
    for _ in range(10):                                   # 1 % N and '-' sprinkled over random records
        b = bytearray(acgt[rng.integers(0, 4, size=int(rng.integers(300, 1500)))])
        for p in rng.integers(0, len(b), size=max(1, len(b) // 100)):
            b[int(p)] = b"N-"[int(rng.integers(0, 2))]
        seqs.append(bytes(b))
    return seqs


def fasta_of(seqs):
    return b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs))


def sequence_lines(fasta):
    return [l for l in fasta.split(b"\n")[:-1] if not l.startswith(b">")]


def split(out_bytes, out_offsets):
    raw = bytes(np.ascontiguousarray(out_bytes, dtype=np.uint8))
    return [raw[int(a):int(b)] for a, b in zip(out_offsets[:-1], out_offsets[1:])]


def pack_like(seqs):
    seqs = list(seqs)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:int(offs[-1])].copy(), offs
