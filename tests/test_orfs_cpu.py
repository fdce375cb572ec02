"""CPU-only checks of `circkit orfs`: the C restatement (tests/orfs_ref.c) against the reference's own unit tests (recorded
in tests/golden/ref_orfs_known_answers.json) and its proptests (lib/src/orfs.rs:571-670, restated as seeded property
tests), and the kernel's per-lane routine (circkit_amd/csrc/orfs.h, built for the host) against the restatement."""
import json
import os
import random

import numpy as np
import pytest

from tests import orfs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def known_answers():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "ref_orfs_known_answers.json")))["cases"]


def orf_seq(seq, start, length):
    """Orf::seq (lib/src/orfs.rs:19-36 with include_stop): `length` bytes cut cyclically from start."""
    return bytes(seq[(start + k) % len(seq)] for k in range(length))


@pytest.mark.parametrize("case", known_answers(), ids=lambda c: c["name"])
def test_restatement_known_answers(case):
    seq = case["seq"].encode()
    exp = [tuple(e) for e in case["expected"]]
    if case["call"] == "longest":
        got = [o[:4] for o in R.orfs_record(seq, strands=1, mode=0)]
    else:
        got = R.find_orfs(seq)
    assert got == exp
    if "expected_seq" in case:
        assert orf_seq(seq, got[0][0], got[0][3]) == case["expected_seq"].encode()


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)[:int(offs[-1])], offs


@pytest.mark.parametrize("case", known_answers(), ids=lambda c: c["name"])
def test_lane_routine_known_answers(case):
    seq = case["seq"].encode()
    d, o = _pack([seq])
    _, got = R.lane_orfs_batch(d, o, strands=1, mode=0 if case["call"] == "longest" else 1)
    got = [(int(g["start"]), None if int(g["stop"]) == R.NONE else int(g["stop"]), int(g["wraps"]), int(g["length"])) for g in got]
    assert got == [tuple(e) for e in case["expected"]]


# ---- the reference's proptests, seeded ("[ATGC]{3,300}") -------------------------------------------------------------
def _random_seqs(seed, n=300):
    rng = random.Random(seed)
    return [bytes(rng.choice(b"ATGC") for _ in range(rng.randint(3, 300))) for _ in range(n)]


def bio_find_all(seq):
    """rust-bio 0.x seq_analysis::orf::Finder(ATG; TAA,TAG,TGA; min_len 0).find_all: a linear scan that keeps the open
    starts of each frame and closes all of them at the frame's next stop.  [(start, end, offset)]."""
    out, open_ = [], [[], [], []]
    for i in range(len(seq) - 2):
        c, f = seq[i:i + 3], i % 3
        if c == b"ATG":
            open_[f].append(i)
        elif c in (b"TAA", b"TAG", b"TGA"):
            out += [(s, i + 3, f) for s in open_[f]]
            open_[f] = []
    return out


def test_property_bio_orfs():
    for seq in _random_seqs(1):
        bio, ck = bio_find_all(seq), R.find_orfs(seq)
        for start, end, off in bio:
            m = [o for o in ck if o[0] == start and o[1] is not None and o[1] + 3 == end]
            assert m, (seq, start, end)
            assert m[0][2] == 0 and m[0][0] % 3 == off
        for o in ck:
            found = any(o[0] == b[0] and (o[1] or 0) + 3 == b[1] for b in bio)
            if o[2] == 0:
                assert found, (seq, o)
            if not found:
                assert o[2] != 0, (seq, o)


def test_property_bio_orfs_repeated():
    for seq in _random_seqs(2, 150):
        dup = seq * 4
        ck = {orf_seq(seq, o[0], o[3]) for o in R.find_orfs(seq)}
        for start, end, _ in bio_find_all(dup):
            assert dup[start:end] in ck, (seq, start, end)


def test_property_no_start_is_its_own_stop_and_lengths_divide_by_three():
    for seq in _random_seqs(3):
        for o in R.find_orfs(seq):
            assert o[1] != o[0]
            assert o[3] % 3 == 0


def test_property_longest_is_a_subset():
    for seq in _random_seqs(4):
        every = R.find_orfs(seq)
        longest = [o[:4] for o in R.orfs_record(seq, strands=1, mode=0)]
        assert len(longest) <= len(every)
        assert all(o in every for o in longest)


# ---- the kernel's per-lane routine against the restatement -----------------------------------------------------------
def adversarial_batch(rng, n=40):
    seqs = []
    for _ in range(n):
        alpha = rng.choice([b"ACGT", b"ATG", b"TAG", b"ATGN-", b"AT", b"ACGTacgt", b"TGA", b"ACGTN"])
        L = rng.choice([rng.randint(0, 12), rng.randint(0, 80), rng.randint(100, 400)])
        seqs.append(bytes(rng.choice(alpha) for _ in range(L)))
    seqs += [b"ATG" + b"C" * 30, b"C" * 31 + b"AT", b"GAT" + b"C" * 25, b"TAATG", b"AT", b"TA", b"ATGATGTAG", b"A", b""]
    return seqs


GRID_CODONS = [(["ATG"], ["TAA", "TAG", "TGA"]), (["ATG", "TAA"], ["TAA", "TAG", "TGA"]), (["ATG", "CTG", "TTG"], ["TAA", "TAG", "TGA"]),
               (["TAG", "ATG", "TGA"], ["TAG"]), (["NNA", "A-G", "AT"], ["TAA", "ATGA"]), (["ATG"], ["ATG", "TAG"])]


def random_params(rng):
    st, sp = rng.choice(GRID_CODONS)
    kw = dict(start_codons=st, stop_codons=sp, min_length=rng.choice([0, 0, 6, 75, 10 ** 9]), min_ratio=rng.choice([0, 0.5, 1, 1.5]),
              min_wraps=rng.randint(0, 3), max_wraps=rng.randint(0, 3), require_stop=rng.random() < 0.5,
              strands=rng.choice([1, 2, 3]), mode=rng.choice([0, 0, 1]))
    if rng.random() < 0.4:
        kw.update(min_length=0, min_ratio=0, min_wraps=0, max_wraps=3)
    return kw


def test_lane_routine_matches_restatement():
    rng = random.Random(7)
    for _ in range(300):
        seqs = adversarial_batch(rng)
        kw = random_params(rng)
        d, o = _pack(seqs)
        eo, e = R.orfs_batch(d, o, **kw)
        go, g = R.lane_orfs_batch(d, o, **kw)
        assert np.array_equal(eo, go), kw
        assert np.array_equal(e, g), kw


def test_lane_routine_every_length_mod_three():
    rng = random.Random(8)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in range(2, 600)]
    seqs += [b"ATG" + bytes(rng.choice(b"ACG") for _ in range(L)) for L in range(0, 200)]       # frames with no stop
    d, o = _pack(seqs)
    for mode in (0, 1):
        for mw in range(4):
            kw = dict(max_wraps=mw, mode=mode, strands=3)
            assert all(np.array_equal(a, b) for a, b in zip(R.orfs_batch(d, o, **kw), R.lane_orfs_batch(d, o, **kw))), kw


def test_ryu_format():
    assert [R.ryu_f64(x) for x in (1.0, 0.5, 0.00012, 1e-7, 3.0, 1e-5, 1.5e-6, 0.1)] == \
        ["1.0", "0.5", "0.00012", "1e-7", "3.0", "0.00001", "1.5e-6", "0.1"]


def test_library_exports_the_orf_entry_points():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    lib = circkit_amd.load_library()
    for s in ("circkit_orfs_batch_device", "circkit_orfs_status", "circkit_orfs_batch", "circkit_find_orfs"):
        assert hasattr(lib, s), s
    p = circkit_amd.orf_params(start_codons=["ATG", "CTG", "AT"], strands="both", mode="all")
    assert (p.n_start_codons, p.n_stop_codons, p.strands, p.mode) == (2, 3, 3, 1)


# ---- the ORF kernels' edges, the emit kernel's sort and the filter boundaries, on the host build -------------------------
CSRC = os.path.join(ROOT, "circkit_amd", "csrc")
# the record counts of tests/test_orfs_gpu_edges.py test_scan_edges_every_record: both sides of a workgroup of the count and
# emit kernels (ORF_WG), of a scan tile (SCAN_TILE records) and of one chunk of SCAN_WG tile sums in scan_sums, then a
# second chunk of one tile and a third chunk
SCAN_COUNTS = [1, 255, 256, 257, 8191, 8192, 8193, 8_388_607, 8_388_608, 8_388_609, 16_777_217]
# the ORFs per strand of sort_switch_records: both sides of sort_run's switch from insertion sort to heapsort, and heapsort
SORT_COUNTS = [31, 32, 33, 64, 3000]


def kernel_constants():
    """ORF_WG, SCAN_WG, SCAN_ITEMS (circkit_orfs.hip), SORT_INSERTION_MAX (orfs.h), and SCAN_TILE = SCAN_WG * SCAN_ITEMS."""
    import re
    src = open(os.path.join(CSRC, "circkit_orfs.hip")).read() + open(os.path.join(CSRC, "orfs.h")).read()
    c = {}
    for name in ("ORF_WG", "SCAN_WG", "SCAN_ITEMS", "SORT_INSERTION_MAX"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m, name
        c[name] = int(m.group(1))
    c["SCAN_TILE"] = c["SCAN_WG"] * c["SCAN_ITEMS"]
    return c


def test_edge_counts_straddle_the_kernel_edges():
    """If a launch or sort constant of the ORF kernels changes, SCAN_COUNTS / SORT_COUNTS above must move with it."""
    c = kernel_constants()
    chunk = c["SCAN_WG"] * c["SCAN_TILE"]
    for name, edge in (("ORF_WG", c["ORF_WG"]), ("SCAN_TILE", c["SCAN_TILE"]), ("one chunk of tile sums", chunk)):
        assert {edge - 1, edge, edge + 1} <= set(SCAN_COUNTS), ("SCAN_COUNTS", name, edge)
    assert 1 in SCAN_COUNTS and 2 * chunk < max(SCAN_COUNTS) <= 2 * chunk + c["SCAN_TILE"], "SCAN_COUNTS: a third chunk"
    b = c["SORT_INSERTION_MAX"]
    assert {b - 1, b, b + 1} <= set(SORT_COUNTS) and max(SORT_COUNTS) > 1000, ("SORT_COUNTS", b)


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def sort_switch_records():
    """Records with runs of exactly SORT_COUNTS ORFs per strand in both modes (min_length 0, no other filter).  Each unit is
    a start with its own stop (ATG TAA, ATG AAA TAA, ATG CCC TGA), 7, 10 or 11 symbols long, so the starts fall in every
    frame and many ORFs share a length across frames: heapsort must break those ties by frame, then start.  Each record
    comes with its reverse complement, which puts the same run on the reverse strand."""
    rng = random.Random(91)
    units = [b"ATGTAAC", b"ATGAAATAAC", b"ATGCCCTGAGG"]
    out = []
    for k in SORT_COUNTS:
        for s in (b"".join(rng.choice(units) for _ in range(k)), units[0] * k):
            out += [s, revcomp(s)]
    return out


def test_lane_sort_switch():
    """sort_run (orfs.h), the emit kernel's sort, through the host build: every run size of SORT_COUNTS on both strands in
    both modes, with length ties across all three frames, against the restatement."""
    seqs = sort_switch_records()
    d, o = _pack(seqs)
    for mode in (0, 1):
        for strands in (1, 2, 3):
            eo, e = R.orfs_batch(d, o, mode=mode, strands=strands)
            go, g = R.lane_orfs_batch(d, o, mode=mode, strands=strands)
            assert np.array_equal(eo, go) and np.array_equal(e, g), (mode, strands)
        runs = {(st, int(np.sum(e["strand"][eo[i]:eo[i + 1]] == st))) for i in range(len(seqs)) for st in (0, 1)}
        for k in SORT_COUNTS:
            assert (0, k) in runs and (1, k) in runs, (mode, k)
        frames = {}
        for i in range(len(seqs)):
            for r in e[eo[i]:eo[i + 1]]:
                frames.setdefault((i, int(r["strand"]), int(r["length"])), set()).add(int(r["start"]) % 3)
        assert any(len(f) == 3 for f in frames.values()), mode


def _around(x):
    import math
    return (math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf))


def filter_boundary_cases():
    """(records, params, chosen (length, L) pairs) at the exact edges of each filter of orfs.h passes(), in both modes.
    The records have prime lengths near 1000, so length / L is not dyadic.  min_ratio sits at length / L (correctly
    rounded) and at its two neighbours for the chosen ORFs; for most of them `length / L >= r` and `length >= r * L`
    disagree at one of the three.  min_length sits at length - 3, one either side of it, and near 2^64.  min_wraps is above
    max_wraps, and max_wraps is 4 and 2^32 - 1."""
    rng = random.Random(101)
    primes = [p for p in range(960, 1300) if all(p % q for q in range(2, 37))][:24]
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(p)) for p in primes]
    d, o = _pack(seqs)
    eo, e = R.orfs_batch(d, o, mode=1)
    pairs = sorted({(int(e["length"][k]), len(seqs[i])) for i in range(len(seqs)) for k in range(int(eo[i]), int(eo[i + 1]))})
    split = [(l, L) for l, L in pairs if any((l / L >= r) != (l >= r * L) for r in _around(l / L))]
    chosen = split[::max(1, len(split) // 6)][:6] + random.Random(102).sample(pairs, 4)
    cases = []
    for mode in (0, 1):
        for l, L in chosen:
            cases += [dict(mode=mode, min_ratio=r) for r in _around(l / L)]
            cases += [dict(mode=mode, min_length=m) for m in (l - 4, l - 3, l - 2) if m >= 0]
        cases += [dict(mode=mode, min_length=m) for m in (2 ** 64 - 3, 2 ** 64 - 2, 2 ** 64 - 1)]
        cases += [dict(mode=mode, min_wraps=a, max_wraps=b) for a, b in ((1, 0), (2, 1), (3, 2), (4, 3), (0, 4), (2, 4),
                                                                          (0, 2 ** 32 - 1), (3, 2 ** 32 - 1), (4, 2 ** 32 - 1))]
    return seqs, cases, chosen


def test_filter_boundaries_are_sharp():
    """The boundary cases are not vacuous: the kept set changes across each ratio and each length boundary, chosen ORFs
    tell `length / L >= r` from `length >= r * L`, and min_length near 2^64 or min_wraps > max_wraps keeps nothing."""
    import math
    seqs, _, chosen = filter_boundary_cases()
    d, o = _pack(seqs)

    def kept(**kw):
        return len(R.orfs_batch(d, o, mode=1, **kw)[1])
    for l, L in chosen:
        r = l / L
        assert r * 2 ** 20 != math.floor(r * 2 ** 20), (l, L)          # not dyadic
        assert kept(min_ratio=r) > kept(min_ratio=math.nextafter(r, math.inf)), (l, L)
        assert kept(min_length=l - 3) > kept(min_length=l - 2), (l, L)
    assert sum(any((l / L >= x) != (l >= x * L) for x in _around(l / L)) for l, L in chosen) >= 5
    assert kept() > 0 and kept(min_length=2 ** 64 - 1) == 0 and kept(min_wraps=2, max_wraps=1) == 0


def test_lane_filter_boundaries():
    seqs, cases, _ = filter_boundary_cases()
    d, o = _pack(seqs)
    for kw in cases:
        eo, e = R.orfs_batch(d, o, **kw)
        go, g = R.lane_orfs_batch(d, o, **kw)
        assert np.array_equal(eo, go) and np.array_equal(e, g), kw


def test_csv_row_and_cyclic_cut():
    """The writer restatements: the csv crate's quoting (oracle.csv_row) and Orf::seq's cyclic cut."""
    from oracle import oracle as O
    assert O.csv_row([b"a", b"", b"b"], b",") == b"a,,b\n"
    assert O.csv_row([b"", b""], b",") == b",\n"
    assert O.csv_row([b"a,b", b'q"t', b"x\ty"], b",") == b'"a,b","q""t",x\ty\n'
    assert O.csv_row([b"a,b", b"x\ty", b"c\rd", b"e\nf"], b"\t") == b'a,b\t"x\ty"\t"c\rd"\t"e\nf"\n'
    assert R.cyclic_cut(b"ABCDE", 3, 12) == b"DEABCDEABCDE"
    assert R.cyclic_cut(b"ABCDE", 7, 2) == b"CD" and R.cyclic_cut(b"ABCDE", 1, 0) == b""
