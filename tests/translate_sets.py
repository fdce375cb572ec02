"""Crafted batches and window lists for the translation of cyclic windows, shared by its CPU fiber test and its GPU test (TEST
INFRASTRUCTURE ONLY).  A case is (name, data, offsets, windows, placement keywords, (aa, unknown, first_as_m)); everything is
seeded."""
import os
import re

import numpy as np

from tests import translate_ref as T
from tests.windows_ref import WINDOW_DTYPE, windows as W
from tests.windows_sets import invalid_rows

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")
RECORD_LENGTHS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 47, 48, 49, 50, 100, 1000]
# three symbols in four are ACGT, so that two codons in five translate; the rest must come out as `unknown` on either strand:
# N, '-', lower case, the IUPAC codes the complement table maps, and bytes it leaves alone
ALPHABET = b"ACGT" * 28 + b"N-acgtnRYKMSWBDHVrykmswbdhv" + bytes([0, 1, 0x7F, 0x80, 0xFE, 0xFF, ord("U"), ord("u"), ord("."), ord("\n")])
WRAP = 2 ** 32 - 1
TABLE_1 = T.genetic_codes()[1]
DISTINCT = bytes(range(0x30, 0x70))                      # 64 different residues: every slip of a codon index shows
CODES = ((TABLE_1, b"X", False), (TABLE_1, b"X", True), (DISTINCT, b"!", False), (DISTINCT, b"!", True))


def constants():
    """The named constants of the translate: its geometry (window_translate.h) and the scan's (circkit_windows.hip)."""
    src = open(os.path.join(CSRC, "window_translate.h")).read() + open(os.path.join(CSRC, "circkit_windows.hip")).read()
    c = {}
    for name in ("TRANSLATE_WAVES", "TRANSLATE_STEPS", "WSCAN_WG", "WSCAN_ITEMS"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, name
        c[name] = int(m.group(1))
    c["TILE_RESIDUES"] = 64 * 16 * c["TRANSLATE_STEPS"] * c["TRANSLATE_WAVES"]
    c["WSCAN_TILE"] = c["WSCAN_WG"] * c["WSCAN_ITEMS"]
    c["WSCAN_CHUNK"] = c["WSCAN_WG"] * c["WSCAN_TILE"]         # windows per round of the single-workgroup second level
    return c


def batch(rng, lengths=RECORD_LENGTHS):
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    data = np.frombuffer(ALPHABET, dtype=np.uint8)[rng.integers(0, len(ALPHABET), size=int(offs[-1]))]
    return data, offs


def window_lengths(n):
    # 3n: the first length at which every codon phase has crossed the origin when 3 does not divide n
    return [0, 1, 2, 3, 4, 5, 47, 48, 49, n - 1, n, n + 1, 2 * n, 3 * n, 3 * n + 1, 4 * n + 5]


def window_starts(n):
    return [0, 1, 2, n - 3, n - 2, n - 1, n, n + 7, WRAP]


def grid(lengths, window_lengths=window_lengths, starts=window_starts):
    """Every (record, window length, start, strand), as rows for windows_ref.windows."""
    rows = []
    for r, n in enumerate(lengths):
        for length in sorted(set(window_lengths(n))):
            for start in sorted(set(starts(n))):
                if length < 0 or start < 0:
                    continue                              # n - 1 of an empty record
                rows += [(length, r, start, 0), (length, r, start, 1)]
    return rows


def main_cases(rng):
    """The full grid over every record; the same record named by many consecutive windows; records in descending order; invalid
    windows between valid ones: once per table and setting of first_as_m."""
    data, offs = batch(rng)
    nr = len(RECORD_LENGTHS)
    rows = grid(RECORD_LENGTHS)
    rows += [(9 + k % 7, 13, 7 * k, k & 1) for k in range(200)]                            # record 13 (100 symbols), 200 times in a row
    rows += [(3, 1, k, k & 1) for k in range(70)]                                         # 70 one-residue windows on the one-symbol record
    rows += [(RECORD_LENGTHS[r] + 4, r, 1, r & 1) for r in range(nr - 1, -1, -1)]          # descending records
    bad = invalid_rows(nr)
    mixed = []
    for k, row in enumerate(grid(RECORD_LENGTHS[:10], lambda n: [n, 3 * n, 50], lambda n: [n + 7])):
        mixed.append(row)
        if k % 3 == 0:
            mixed.append(bad[(k // 3) % len(bad)])
    wins = W(rows + mixed)
    return [("grid, code %d" % k, data, offs, wins, {}, code) for k, code in enumerate(CODES)]


def shift_cases(rng):
    """A reduced set at every payload shift and every output shift mod 16: 16 passes, each shift once on either side."""
    lengths = [0, 1, 2, 4, 16, 17, 50, 100]
    data, offs = batch(rng, lengths)
    rows = grid(lengths, lambda n: [3, 48, 49, n + 1, 3 * n], lambda n: [0, n - 2, n + 7]) + invalid_rows(len(lengths))[:2]
    wins = W(rows)
    return [("shift %d" % s, data, offs, wins, dict(in_shift=s, out_shift=(7 * s + 3) % 16, lead=s % 5), CODES[s % 4]) for s in range(16)]


def boundary_cases(rng, c):
    """Window counts on both sides of a scan tile; total residues and window counts on both sides of a translate tile; one window
    that spans several tiles, on either strand."""
    data, offs = batch(rng)
    nr = len(RECORD_LENGTHS)
    out = []
    for count in (c["WSCAN_TILE"] - 1, c["WSCAN_TILE"], c["WSCAN_TILE"] + 1, 2 * c["WSCAN_TILE"] + 1):
        w = np.zeros(count, dtype=WINDOW_DTYPE)
        w["length"] = rng.integers(0, 30, size=count)
        w["record"] = rng.integers(0, nr + 1, size=count)                                # (record nr: invalid)
        w["start"] = rng.integers(0, 2 ** 32, size=count)
        w["strand"] = rng.integers(0, 2, size=count)
        out.append(("scan count %d" % count, data, offs, w, dict(out_shift=count % 16), CODES[count % 4]))
    per = c["TILE_RESIDUES"] // 16
    for count, last in ((per - 1, 16), (per, 15), (per, 16), (per, 17), (per + 1, 16)):
        rows = [(48 + k % 3, 6 + k % 9, 3 * k, k & 1) for k in range(count - 1)] + [(3 * last + 2, 14, 990, 1)]
        out.append(("tile: %d windows, the last of %d" % (count, last), data, offs, W(rows), {}, CODES[(count + last) % 4]))
    big = 3 * (2 * c["TILE_RESIDUES"] + 1234) + 1
    out.append(("a window across tiles", data, offs, W([(9, 3, 1, 0), (big, 14, 999, 0), (3, 1, 0, 1), (big, 13, 5, 1), (6, 2, 0, 0)]),
                dict(in_shift=9, out_shift=6, lead=2), CODES[3]))
    return out


def all_cases(c=None):
    c = c or constants()
    rng = np.random.default_rng(2026)
    return main_cases(rng) + shift_cases(rng) + boundary_cases(rng, c)


def expected(case):
    name, data, offs, wins, _, (aa, unknown, first_as_m) = case
    return T.windows_translate(data, offs, wins, aa, unknown, first_as_m)
