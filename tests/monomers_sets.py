"""Crafted batches for the monomer compact, shared by its CPU fiber test and its GPU test (TEST INFRASTRUCTURE ONLY).  A case
is (name, data, offsets, ends, full_len | None, filter keywords); the end indices are crafted, so no monomerize run is
needed.  Everything is seeded.  TILE = the gather's output tile in bytes (monomer_compact.h TILE_BYTES)."""
import re
import os

import numpy as np

NONE = 0xFFFFFFFF
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")


def constants():
    """The named constants of the compact: the gather's geometry (monomer_compact.h) and the scan's (circkit_monomerize.hip)."""
    src = open(os.path.join(CSRC, "monomer_compact.h")).read() + open(os.path.join(CSRC, "circkit_monomerize.hip")).read()
    c = {}
    for name in ("GATHER_WAVES", "GATHER_STEPS", "COMPACT_WG", "CSCAN_WG", "CSCAN_ITEMS"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, name
        c[name] = int(m.group(1))
    c["STEP_BYTES"] = 64 * 16
    c["WAVE_BYTES"] = c["STEP_BYTES"] * c["GATHER_STEPS"]
    c["TILE_BYTES"] = c["WAVE_BYTES"] * c["GATHER_WAVES"]
    c["CSCAN_TILE"] = c["CSCAN_WG"] * c["CSCAN_ITEMS"]
    c["CSCAN_CHUNK"] = c["CSCAN_WG"] * c["CSCAN_TILE"]         # records per round of the single-workgroup second level
    return c


def batch(rng, lengths, alpha=None):
    """Random records of the given lengths: (data, offsets).  Every byte value occurs unless alpha is given."""
    lengths = np.asarray(lengths, dtype=np.int64)
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    total = int(offs[-1])
    if alpha is None:
        data = rng.integers(0, 256, size=total, dtype=np.uint8)
    else:
        data = np.frombuffer(alpha, dtype=np.uint8)[rng.integers(0, len(alpha), size=total)]
    return data, offs


def ends_of(lengths, written):
    """End indices that write `written[i]` bytes of record i (None = drop: NONE)."""
    return np.array([NONE if w is None else w for w in written], dtype=np.uint32)


def case(name, rng, lengths, written, full_len=None, **filter):
    data, offs = batch(rng, lengths)
    return (name, data, offs, ends_of(lengths, written), full_len, filter)


def emulator_sets(tile):
    """The sets of the issue's emulator list."""
    rng = np.random.default_rng(2024)
    out = []
    # every written length 0..300, of records a little longer than that
    w = list(range(301))
    out.append(case("every written length", rng, [x + x % 7 for x in w], w))
    out.append(case("every written length, downwards, whole records", rng, w[::-1], w[::-1]))
    # granules that hold three and more records: lengths 0..5, with drops
    ln = rng.integers(0, 6, size=700).tolist()
    out.append(case("tiny records", rng, ln, ln))
    out.append(case("tiny records, a third dropped", rng, ln, [None if i % 3 == 1 else x for i, x in enumerate(ln)]))
    # runs of empty records under keep_all: None and n = 0, between written ones
    ln = [3, 0, 0, 0, 0, 0, 0, 5, 0, 1, 0, 0, 0] * 20 + [0] * 70 + [2] + [0] * 70
    out.append(case("runs of empty records, keep_all", rng, ln, [None if x == 0 or i % 5 == 0 else x for i, x in enumerate(ln)], keep_all=True))
    out.append(case("only empty records, keep_all", rng, [0] * 100, [None] * 100, keep_all=True))
    # first, last or all records dropped, and all kept
    ln = rng.integers(1, 90, size=60).tolist()
    out.append(case("first dropped", rng, ln, [None] + ln[1:]))
    out.append(case("last dropped", rng, ln, ln[:-1] + [None]))
    out.append(case("all dropped", rng, ln, [None] * len(ln)))
    out.append(case("all kept", rng, ln, ln))
    out.append(case("all kept as prefixes", rng, ln, [x // 2 for x in ln]))
    out.append(case("only the last written", rng, ln, [None] * (len(ln) - 1) + ln[-1:]))
    out.append(case("none found, keep_all", rng, ln, [None] * len(ln), keep_all=True))
    # one monomer that spans several output tiles, tiny ones on both sides
    big = 2 * tile + 1234
    out.append(case("a monomer across tiles", rng, [1, 2, 0, 3, big + 50, 1, 1, 2], [1, 2, 0, 3, big, 1, None, 2]))
    # a tile boundary on a record boundary, and one byte on either side; the same for a wave's share and for a step
    for edge, what in ((tile, "tile"), (tile // 4, "wave"), (1024, "step")):
        for d in (-1, 0, 1):
            first = edge + d
            out.append(case("%s boundary %+d" % (what, d), rng, [first + 9, 40, 1, edge, 17], [first, 40, 1, edge, 17]))
    # the last record's last 16 bytes, and the first record's first: whole records at both ends of the payload
    for last in (1, 2, 15, 16, 17, 31, 33):
        out.append(case("last record of %d bytes" % last, rng, [37, 5, last], [37, 5, last]))
        out.append(case("first record of %d bytes" % last, rng, [last, 5, 37], [last, 5, 37]))
    for total in (1, 5, 15, 16):                 # a payload of no more than a granule
        out.append(case("payload of %d bytes" % total, rng, [total], [total]))
        out.append(case("payload of %d bytes in single bytes" % total, rng, [1] * total, [1] * total))
    return out


def misalignment_set():
    """The short set of the 16 x 16 source / destination misalignments: a dropped record in front moves the source of
    everything behind it, prefixes move it again."""
    rng = np.random.default_rng(77)
    ln = [5, 40, 3, 0, 100, 16, 17, 1, 33, 64, 15, 250]
    wr = [None, 40, 2, 0, 77, 16, None, 1, 32, 64, 15, 249]
    return case("misalignment", rng, ln, wr)


def filter_boundary_cases():
    """(name, lengths, ends, full_len, filter, expected kept) on crafted (n, f, end) triples, at each filter's exact edge."""
    out = []
    n, f, idx = 100, 130, 60

    def one(name, kept, n_=n, f_=f, e_=idx, **flt):
        out.append((name, [n_], [e_], [f_], flt, kept))
    for d in (-1, 0, 1):
        one("min_length idx%+d" % d, d <= 0, min_length=idx + d)
        one("max_length idx%+d" % d, d >= 0, max_length=idx + d)
    one("min_overlap f-idx", True, min_overlap=f - idx)
    one("min_overlap f-idx+1", False, min_overlap=f - idx + 1)
    # exact ratios: (f - idx) / idx = 0.5, 1.0, 1.5
    for num, ratio in ((30, 0.5), (60, 1.0), (90, 1.5)):
        for thr, kept in ((ratio, True), (np.nextafter(ratio, 2.0), False), (np.nextafter(ratio, 0.0), True)):
            one("percent %r vs %r" % (ratio, float(thr)), kept, n_=150, f_=60 + num, e_=60, min_overlap_percent=float(thr))
    # a ratio that is not representable: 51 / 100 in f64 against 0.51 and its two neighbours
    q = float(np.float64(51.0) / np.float64(100.0))
    for thr in (float(np.nextafter(0.51, 0.0)), 0.51, float(np.nextafter(0.51, 1.0))):
        one("percent 51/100 vs %r" % thr, not (q < thr), n_=151, f_=151, e_=100, min_overlap_percent=thr)
    for thr in (float("nan"), 0.0, -1.0):
        one("percent %r" % thr, True, min_overlap_percent=thr)
        one("percent %r, idx 0" % thr, True, e_=0, min_overlap_percent=thr)       # x / 0: inf, never below
        one("percent %r, idx 0 of an empty record" % thr, True, n_=0, f_=0, e_=0, min_overlap_percent=thr)      # 0 / 0: NaN
    one("f > n: the overlap counts the stripped bytes", True, n_=100, f_=140, e_=60, min_overlap=80)
    one("f > n, one more", False, n_=100, f_=140, e_=60, min_overlap=81)
    one("f < n saturates", False, n_=100, f_=50, e_=60, min_overlap=1)
    one("end == n", True, e_=n)
    one("end > n", False, e_=n + 1)
    one("end far beyond n", False, e_=0xFFFFFFFE)
    one("end NONE", False, e_=NONE)
    return out
