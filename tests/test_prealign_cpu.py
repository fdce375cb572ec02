"""CPU-only: the prealign surface of the ABI, the yardstick tests/prealign_ref.py against hand-worked answers of the definition, the
condition on the planted set, and the device routines of circkit_amd/csrc/prealign.h and the anchor routines of sketch.h run as
fibers by a stand-alone program (tests/emu/prealign_emu_main.cpp) against the yardstick: every anchor, row, count, window, score
and total."""
import ctypes

import numpy as np
import pytest

from tests import prealign_ref as P
from tests import prealign_sets as S
from tests import sketch_ref as R

NAMES = {"circkit_sketch_anchors_device": 8, "circkit_prealign_pairs_device": 10, "circkit_prealign_status": 3,
         "circkit_prealign_pairs_of_labels_device": 4, "circkit_prealign_batch": 10}
INVALID_ARG = -1
NONE = P.NONE


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------
def test_the_surface():
    import os
    import re
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    from circkit_amd import api
    from tests.test_abi import ROOT, header_symbols
    lib = circkit_amd.load_library()
    syms = header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = set(re.findall(r"pub fn (circkit_[a-z0-9_]+)\s*\(", text[text.index("## 2. Declarations"):text.index("## 3. Drop-in")]))
    for name, n_args in NAMES.items():
        assert name in syms, "include/circkit.h does not declare %s" % name
        assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), "libcirckit_hip.so does not export %s" % name
        assert name in bound, "INTEGRATION.md does not bind %s" % name
    for method in ("sketch_anchors_device", "prealign_pairs_device", "prealign_status", "prealign_pairs_of_labels_device", "prealign_batch"):
        assert callable(getattr(api.Context, method))
    for fn in ("prealign_params", "sketch_anchors", "prealign_batch"):
        assert callable(getattr(circkit_amd, fn))
    assert callable(circkit_amd.prealign.prealign_fasta)
    assert ctypes.sizeof(api.PrealignParams) == 16
    p = circkit_amd.prealign_params()
    assert (p.k, p.log2_bins, p.min_votes, p.reserved) == (21, 8, 4, 0)
    p = circkit_amd.prealign_params(k=4, log2_bins=10, min_votes=1)
    assert (p.k, p.log2_bins, p.min_votes, p.reserved) == (4, 10, 1, 0)
    assert circkit_amd.ANCHOR_NONE == api.ANCHOR_NONE == NONE
    header = open(os.path.join(ROOT, "include", "circkit.h")).read()
    assert re.search(r"uint32_t k;[^}]*?uint32_t log2_bins;[^}]*?uint32_t min_votes;[^}]*?uint32_t reserved;[^}]*?\} circkit_prealign_params;", header, flags=re.S)
    assert re.search(r"#define CIRCKIT_ANCHOR_NONE 0xFFFFFFFFu", header)
    assert api.WINDOW_DTYPE == P.WINDOW_DTYPE


def test_a_null_ctx_is_refused_without_a_device():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    lib = circkit_amd.load_library()
    p = circkit_amd.prealign_params()
    sp = circkit_amd.sketch_params()
    t = ctypes.c_uint64(7)
    out = (ctypes.c_uint32 * 8)(*([9] * 8))
    assert lib.circkit_sketch_anchors_device(None, None, None, 0, ctypes.byref(sp), None, None, out) == INVALID_ARG
    assert lib.circkit_prealign_pairs_device(None, None, None, None, 0, ctypes.byref(p), None, 0, out, out) == INVALID_ARG
    assert lib.circkit_prealign_status(None, ctypes.byref(t), ctypes.byref(t)) == INVALID_ARG
    assert lib.circkit_prealign_pairs_of_labels_device(None, None, 0, out) == INVALID_ARG
    assert lib.circkit_prealign_batch(None, None, None, 0, ctypes.byref(sp), None, 0, 4, out, out) == INVALID_ARG
    assert t.value == 7 and list(out) == [9] * 8


def test_the_command_line_without_a_device(tmp_path):
    from circkit_amd import prealign
    a = prealign._parser().parse_args([])
    assert (a.input, a.output, a.k, a.bins, a.bands, a.band_bins, a.min_similarity, a.min_votes, a.table) == (None, None, 21, 256, 64, 2, 0.2, 4, None)
    a = prealign._parser().parse_args(["-i", "in.fa", "-o", "out.fa", "--k", "15", "--bins", "64", "--bands", "16", "--band-bins", "4",
                                       "--min-similarity", "0.5", "--min-votes", "9", "--table", "t.tsv"])
    assert (a.input, a.output, a.k, a.bins, a.bands, a.band_bins, a.min_similarity, a.min_votes, a.table) == ("in.fa", "out.fa", 15, 64, 16, 4, 0.5, 9, "t.tsv")
    for bins in ("100", "0"):
        with pytest.raises(SystemExit) as e:
            prealign.main(["--bins", bins])
        assert e.value.code == 2
    assert prealign.main(["-i", str(tmp_path / "missing.fasta")]) == 1
    assert prealign._word(b"rec7 some words") == b"rec7" and prealign._word(b"") == b""
    assert prealign.TITLE == b"record\trepresentative\tstrand\tstart\tvotes\tmatches\n"


# ---- 2. the yardstick --------------------------------------------------------------------------------------------------------
#   ACGAACGATTGC, k = 4: the twelve cyclic k-mers, the reverse complement of each, the smaller of the two and whether it is the
#   reverse complement (o).  Start 4 repeats start 0; start 9 is its own reverse complement; starts 10 and 11 wrap.
TWELVE = b"ACGAACGATTGC"
TWELVE_KMERS = [(0, "ACGA", "TCGT", "ACGA", 0), (1, "CGAA", "TTCG", "CGAA", 0), (2, "GAAC", "GTTC", "GAAC", 0), (3, "AACG", "CGTT", "AACG", 0),
                (4, "ACGA", "TCGT", "ACGA", 0), (5, "CGAT", "ATCG", "ATCG", 1), (6, "GATT", "AATC", "AATC", 1), (7, "ATTG", "CAAT", "ATTG", 0),
                (8, "TTGC", "GCAA", "GCAA", 1), (9, "TGCA", "TGCA", "TGCA", 0), (10, "GCAC", "GTGC", "GCAC", 0), (11, "CACG", "CGTG", "CACG", 0)]


def _base4(word):
    v = 0
    for ch in word:
        v = 4 * v + "ACGT".index(ch)
    return v


@pytest.mark.parametrize("log2_bins,seed", [(4, 0), (5, 99)])
def test_twelve_symbols_by_hand(log2_bins, seed):
    doubled = (TWELVE + TWELVE).decode()
    for p, fwd, rc, canon, o in TWELVE_KMERS:                # the table is the record's
        assert doubled[p:p + 4] == fwd and R.revcomp(fwd.encode()).decode() == rc and canon == min(fwd, rc) and o == (rc < fwd)
    bins = 1 << log2_bins
    row, anc = [P.EMPTY] * bins, [NONE] * bins
    for p, _, _, canon, o in TWELVE_KMERS:                   # ascending p: a later equal hash does not replace the anchor
        h = R.fmix64(_base4(canon) ^ seed)
        b = h >> (64 - log2_bins)
        if h < row[b]:
            row[b], anc[b] = h, 2 * p + o
    got_row, got_n, got_anc = P.anchors(TWELVE, 4, log2_bins, seed)
    assert (got_row, got_n, got_anc) == (row, 12, anc)
    assert 8 not in anc                                       # start 4 never wins: start 0 holds the same k-mer
    assert got_row == R.sketch(TWELVE, 4, log2_bins, seed)[0]


def test_one_pair_by_hand():
    E = P.EMPTY
    #        bin      0   1   2   3   4   5   6   7
    row_a = [100, 101, 102, 103, 104, 105, 106, E]
    row_b = [100, 101, 102, 103, 104, 105, 999, E]
    anc_a = [2 * 3 + 0, 2 * 7 + 1, 2 * 1 + 0, 2 * 8 + 1, 2 * 0 + 0, 2 * 12 + 0, 2 * 1, NONE]
    anc_b = [2 * 5 + 0, 2 * 9 + 1, 2 * 2 + 1, 2 * 9 + 0, 2 * 3 + 1, 2 * 4 + 0, 2 * 1, NONE]
    # n_b = 10, k = 4.  bin 0: s = 0, (5 - 3) = 2.  bin 1: s = 0, (9 - 7) = 2.  bin 2: s = 1, pb = 10 - 2 - 4 = 4, (4 - 1) = 3.
    # bin 3: s = 1, pb = (10 - 9 - 4) mod 10 = 7, (7 - 8) mod 10 = 9.  bin 4: s = 1, pb = 10 - 3 - 4 = 3, (3 - 0) = 3.
    # bin 5: s = 0, pa = 12 > n_b, (4 - 12) mod 10 = 2.  bin 6: the rows differ.  bin 7: empty.
    keys, matches = P.vote_keys(row_a, anc_a, row_b, anc_b, 10, 4)
    assert keys == [2, 2, 0x80000003, 0x80000009, 0x80000003, 2] and matches == 6
    assert P.pair(row_a, anc_a, row_b, anc_b, 10, 1, 4, 3) == ((10, 1, 2, 0, 0), (3, 6), True)
    assert P.pair(row_a, anc_a, row_b, anc_b, 10, 1, 4, 4) == ((10, 1, 0, 0, 0), (3, 6), False)
    # without bin 5 the keys 2 and 0x80000003 tie at two votes: the smaller key, strand 0, wins
    anc_a[5] = NONE
    assert P.pair(row_a, anc_a, row_b, anc_b, 10, 1, 4, 2) == ((10, 1, 2, 0, 0), (2, 5), True)
    # without bin 0 as well the key 0x80000003 stands alone with two
    anc_b[0] = NONE
    assert P.pair(row_a, anc_a, row_b, anc_b, 10, 1, 4, 2) == ((10, 1, 3, 1, 0), (2, 4), True)
    # two starts of one strand tie: the smaller start
    assert P.pair([1, 2, 3, 4], [0, 0, 0, 0], [1, 2, 3, 4], [2 * 6, 2 * 6, 2 * 5, 2 * 5], 10, 0, 4, 1)[0] == (10, 0, 5, 0, 0)
    # no length, no vote; the matches are counted all the same
    assert P.pair(row_a, anc_a, row_b, anc_b, 0, 1, 4, 1) == ((0, 1, 0, 0, 0), (0, 4), False)
    assert P.pair(row_a, anc_a, row_b, anc_b, 2 ** 31, 1, 4, 1) == ((2 ** 31, 1, 0, 0, 0), (0, 4), False)
    w, sc, n_al, n_bad = P.pairs(np.array([row_a, row_b], dtype=np.uint64), np.array([anc_a, anc_b], dtype=np.uint32), [10, 10], 4, 2, [(0, 1), (2, 1), (0, 5)])
    assert [tuple(int(v) for v in x) for x in w] == [(10, 1, 3, 1, 0), (0, 1, 0, 0, 0), (0, 5, 0, 0, 0)] and (n_al, n_bad) == (1, 2)
    assert sc.tolist() == [[2, 4], [0, 0], [0, 0]]
    assert P.pairs_of_labels([0, 0, 2 ** 32, 2 ** 32 - 1]).tolist() == [[0, 0], [0, 1], [NONE, 2], [NONE, 3]]


def test_the_flip_on_a_record_and_its_reverse_complement():
    s = b"ACGGTCATTGCAGCCTAGATCGGATTACCA"
    k, lb, n = 6, 5, 30
    kmers = {min(w, R.revcomp(w)) for w in ((s + s)[p:p + k] for p in range(n))}
    assert len(kmers) == n                                    # no k-mer twice on either strand: every shared bin must agree
    row, _, anc = P.anchors(s, k, lb)
    rc = R.revcomp(s)
    for r in (0, 1, 7, 29):
        t = S.rotate(rc, r)
        row_t, _, anc_t = P.anchors(t, k, lb)
        assert row_t == row
        filled = sum(v != P.EMPTY for v in row)
        # revcomp(t) read from start r is s: the k-mer at p of s starts at (n - p - k) mod n of rc
        assert P.pair(row, anc, row_t, anc_t, n, 1, k, 1) == ((n, 1, r, 1, 0), (filled, filled), True)
        w = np.array([(n, 1, r, 1, 0)], dtype=P.WINDOW_DTYPE)[0]
        assert P.window_bytes([s, t], w) == s
        u = S.rotate(s, r)                                    # and the plain rotation: strand 0
        row_u, _, anc_u = P.anchors(u, k, lb)
        assert P.pair(row, anc, row_u, anc_u, n, 1, k, 1) == ((n, 1, (n - r) % n, 0, 0), (filled, filled), True)


def test_the_sets_hold_what_they_name():
    c = S.constants()
    cases = S.anchor_cases()
    seqs, k, lb, _, _ = cases["wrap"]
    assert any(a != NONE and (a >> 1) > len(seqs[0]) - k for a in S.expected_anchors("wrap")[2][0])
    rows, counts, anc = S.expected_anchors("ties")
    assert counts[0] == 280 and all(a == NONE or (a >> 1) < 7 for a in anc[0])          # 40 copies of 7 symbols: a start below 7 wins
    assert np.array_equal(rows[1], rows[2]) and np.array_equal(anc[1], anc[2])          # the record twice in a row: the first copy's starts
    rows, counts, anc = S.expected_anchors("no_kmers")
    assert (counts == 0).all() and (anc == NONE).all() and (rows == P.EMPTY).all()
    rows, counts, anc = S.expected_anchors("two_spans")
    assert (anc[0][anc[0] != NONE] >> 1).max() < 3000 and len(cases["two_spans"][0][0]) > 2 * c["SKETCH_SEG"]
    assert cases["lead"][4] != 0
    pal = set(int(a) for a in S.expected_anchors("palindrome")[2][1])                     # ACGCGT alone: starts 0 (ACGCGT) and 3 (CGTACG) are
    assert 0 in pal and not pal & {1, 7}                                                  # their own reverse complements: o = 0
    g = S.anchor_grid_cases()
    assert len(g["past_short_grid"][0]) == c["SHORT_MAX_GRID"] * c["SKETCH_WAVES"] + 1
    assert sum(len(s) > c["SKETCH_SEG"] for s in g["past_long_grid"][0]) == c["LONG_GRID"] + 1
    assert len(S.past_the_pairs_grid()[5]) == c["PAIRS_MAX_GRID"] * c["PREALIGN_WAVES"] + 1
    v = {name: S.expected_votes(name) for name in S.vote_cases()}
    w, sc, al, bad = v["tie_two_keys"]
    assert tuple(w[0]) == (50, 1, 2, 0, 0) and sc[0].tolist() == [3, 6]
    w, sc, al, bad = v["tie_strands"]
    assert tuple(w[0]) == (50, 1, 9, 0, 0) and sc[0].tolist() == [3, 6]
    assert v["all_distinct"][1][0].tolist() == [1, 16] and v["one_key_16"][1][0].tolist() == [16, 16]
    assert tuple(v["one_key_1024"][0][0]) == (4000, 1, 3999, 0, 0) and v["one_key_1024"][1][0].tolist() == [1024, 1024]
    assert v["votes_eq_min"][2] == 1 and v["votes_below_min"][2] == 0 and v["votes_eq_min"][1][0].tolist() == [6, 10]
    assert tuple(v["pa_exceeds_nb"][0][0]) == (100, 1, 42, 0, 0)
    assert tuple(v["nb_eq_k"][0][0])[:2] == (8, 1) and v["nb_eq_k"][2] == 1
    assert tuple(v["nb_zero"][0][0]) == (0, 1, 0, 0, 0) and v["nb_zero"][1][0].tolist() == [0, 16]
    assert tuple(v["nb_too_long"][0][0]) == (2 ** 31, 1, 0, 0, 0)
    assert v["none_anchor"][1][0].tolist()[1] == 11
    w, sc, al, bad = v["rotations"]
    for i in range(120):                                      # every rotation and either strand is found exactly
        assert (int(w[i]["start"]), int(w[i]["strand"])) == S.planted_window(60, i % 60, i // 60), i
    w, sc, al, bad = v["self_pairs"]
    assert all((int(x["start"]), int(x["strand"])) == (0, 0) for x in w) and (sc[:, 0] == sc[:, 1]).all() and al == 9
    assert v["invalid"][3] == 5 and v["no_records"][3] == 2
    assert v["random_1024"][1][:, 0].max() > 3


def test_the_planted_set_in_the_yardstick():
    """Every copy against its founder gives the planted strand AND start; the window cut there differs from the founder in exactly
    the planted substitutions; every unrelated pair is unaligned at min_votes = 4."""
    records, plants = S.planted()
    assert len(records) == 160 and len(plants) == 120 and all(300 <= len(r) <= 1500 for r in records)
    k, lb, mv = 21, 8, 4
    rows, _, anc = P.anchors_batch(records, k, lb)
    lengths = [len(r) for r in records]
    fewest = 10 ** 9
    for fi, ci, r, s, subs in plants:
        n = lengths[fi]
        w, (votes, matches), aligned = P.pair(rows[fi], anc[fi], rows[ci], anc[ci], n, ci, k, mv)
        assert aligned and (w[2], w[3]) == S.planted_window(n, r, s), (fi, ci)
        cut = P.window_bytes(records, np.array([w], dtype=P.WINDOW_DTYPE)[0])
        assert [p for p in range(n) if cut[p] != records[fi][p]] == subs, (fi, ci)
        fewest = min(fewest, votes)
    assert fewest == 135                                      # of 256 bins, at 1 % substitutions
    family = np.repeat(np.arange(40), 4)
    for a in range(160):                                      # votes <= matches: only a pair that shares a bin can have a vote
        shared = ((rows == rows[a]) & (rows != np.uint64(P.EMPTY))).sum(axis=1)
        for b in np.flatnonzero((family != family[a]) & (shared > 0)):
            assert not P.pair(rows[a], anc[a], rows[b], anc[b], lengths[b], int(b), k, mv)[2], (a, b)


# ---- 3. the routines as fibers -----------------------------------------------------------------------------------------------
def test_constants():
    from tests.emu import prealign_emu
    c = S.constants()
    assert prealign_emu.constants() == (c["SKETCH_SEG"], c["SKETCH_WAVES"], c["PREALIGN_WAVES"])


def _check_anchors(name, got, want_counts):
    rows, counts, anc = S.expected_anchors(name)
    g_rows, g_anc, g_counts, (valid, unprocessed, n_long) = got
    assert np.array_equal(g_rows, rows), name
    assert np.array_equal(g_anc, anc), name
    if want_counts:
        assert np.array_equal(g_counts, counts), name
    seg = S.constants()["SKETCH_SEG"]
    assert (valid, unprocessed, n_long) == (int(counts.sum()), 0, sum(len(s) > seg for s in S.anchor_cases()[name][0])), name


def test_anchors_as_fibers(tmp_path):
    from tests.emu import prealign_emu
    names = sorted(S.anchor_cases())
    # the grids: two workgroups over the records and three over the long list (fewer long records than workgroups, more, as many)
    cases = [S.anchor_cases()[n] + (2, 3, i % 2 == 0) for i, n in enumerate(names)]
    cases += [S.anchor_cases()["lengths"] + (1, 1, True), S.anchor_cases()["lengths"] + (5, 5, False)]
    got = prealign_emu.run_anchors(cases, tmp_path)
    for i, n in enumerate(names):
        _check_anchors(n, got[i], i % 2 == 0)
    _check_anchors("lengths", got[-2], True)
    _check_anchors("lengths", got[-1], False)


def _check_votes(name, got):
    w, sc, al, bad = S.expected_votes(name)
    assert np.array_equal(got[0], w), name
    assert np.array_equal(got[1], sc), name
    assert (got[2], got[3]) == (al, bad), name


def test_votes_as_fibers(tmp_path):
    from tests.emu import prealign_emu
    names = sorted(S.vote_cases())
    cases = []
    for n in names:
        rows, anc, lengths, k, mv, pairs = S.vote_cases()[n]
        cases.append((rows, anc, S.offsets_of(lengths), k, mv, pairs, 3))
    got = prealign_emu.run_votes(cases, tmp_path)
    for n, g in zip(names, got):
        _check_votes(n, g)


def test_labels_as_fibers(tmp_path):
    from tests.emu import prealign_emu
    names = ["plain", "wide", "empty"]
    got = prealign_emu.run_labels([(S.label_cases()[n], 2) for n in names] + [(np.arange(300, dtype=np.uint64) // np.uint64(3), 2)], tmp_path)
    for n, g in zip(names, got):
        assert np.array_equal(g, P.pairs_of_labels(S.label_cases()[n])), n
    assert np.array_equal(got[-1], P.pairs_of_labels(np.arange(300) // 3))


def test_the_planted_set_as_fibers(tmp_path):
    """Five founders and their copies (the fibers are slow): anchors from the bytes, then every copy against its founder and the
    founders against each other."""
    from tests.emu import prealign_emu
    records, plants = S.planted()
    records, plants = records[:20], plants[:15]
    k, lb = 21, 8
    rows, counts, anc = P.anchors_batch(records, k, lb)
    g_rows, g_anc, g_counts, _ = prealign_emu.run_anchors([(records, k, lb, 0, 0, 3, 2, True)], tmp_path)[0]
    assert np.array_equal(g_rows, rows) and np.array_equal(g_anc, anc) and np.array_equal(g_counts, counts)
    pairs = [(fi, ci) for fi, ci, _, _, _ in plants] + [(a, b) for a in range(0, 20, 4) for b in range(0, 20, 4)]
    lengths = [len(r) for r in records]
    w, sc, al, bad = P.pairs(rows, anc, lengths, k, 4, pairs)
    g = prealign_emu.run_votes([(g_rows, g_anc, S.offsets_of(lengths), k, 4, pairs, 4)], tmp_path)[0]
    assert np.array_equal(g[0], w) and np.array_equal(g[1], sc) and (g[2], g[3]) == (al, bad)
    assert al == 15 + 5
