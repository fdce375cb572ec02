"""CPU-only: the distance surface of the ABI, the yardstick tests/distance_ref.py against answers worked out by hand, the conditions
the sets of tests/distance_sets.py must meet, and the device routines of circkit_amd/csrc/distance.h run as fibers by a stand-alone
program (tests/emu/distance_emu_main.cpp) against the yardstick: every distance, score and total."""
import ctypes

import numpy as np
import pytest

from tests import distance_ref as D
from tests import distance_sets as S

NAMES = {"circkit_distance_pairs_device": 12, "circkit_distance_status": 3, "circkit_distance_pairs": 12}
INVALID_ARG = -1
OVER = D.OVER


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------
def test_the_surface():
    import os
    import re
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    from circkit_amd import api
    from circkit_amd import build as B
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
    for method in ("distance_pairs_device", "distance_status", "distance_pairs"):
        assert callable(getattr(api.Context, method))
    for fn in ("distance_params", "edit_distances"):
        assert callable(getattr(circkit_amd, fn))
    assert "circkit_distance.hip" in B.HIP_SOURCES
    assert ctypes.sizeof(api.DistanceParams) == 16
    p = circkit_amd.distance_params()
    assert (p.max_distance, list(p.reserved)) == (32, [0, 0, 0])
    assert circkit_amd.distance_params(max_distance=255).max_distance == 255
    assert circkit_amd.DISTANCE_OVER == api.DISTANCE_OVER == OVER == 0xFFFFFFFF and circkit_amd.DISTANCE_MAX == D.DISTANCE_MAX == 255
    header = open(os.path.join(ROOT, "include", "circkit.h")).read()
    assert re.search(r"uint32_t max_distance;[^}]*?uint32_t reserved\[3\];[^}]*?\} circkit_distance_params;", header, flags=re.S)
    assert re.search(r"#define CIRCKIT_DISTANCE_OVER 0xFFFFFFFFu", header) and re.search(r"#define CIRCKIT_DISTANCE_MAX 255u", header)


def test_a_null_ctx_is_refused_without_a_device():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    lib = circkit_amd.load_library()
    p = circkit_amd.distance_params()
    t = ctypes.c_uint64(7)
    out = (ctypes.c_uint32 * 8)(*([9] * 8))
    assert lib.circkit_distance_pairs_device(None, None, None, 0, None, None, 0, ctypes.byref(p), None, 0, out, out) == INVALID_ARG
    assert lib.circkit_distance_status(None, ctypes.byref(t), ctypes.byref(t)) == INVALID_ARG
    assert lib.circkit_distance_pairs(None, None, None, 0, None, None, 0, ctypes.byref(p), None, 0, out, out) == INVALID_ARG
    assert t.value == 7 and list(out) == [9] * 8


def test_the_command_lines_without_a_device():
    from circkit_amd import cluster, prealign
    a = cluster._parser().parse_args([])
    assert (a.min_identity, a.max_distance) == (None, None)
    a = cluster._parser().parse_args(["--min-identity", "0.97", "--max-distance", "64"])
    assert (a.min_identity, a.max_distance) == (0.97, 64)
    for argv in (["--min-identity", "0.9"], ["--max-distance", "9"]):       # one without the other
        with pytest.raises(SystemExit) as e:
            cluster.main(argv)
        assert e.value.code == 2
    with pytest.raises(ValueError):
        cluster.cluster_fasta(b">a\nACGT\n", max_distance=3)
    assert prealign._parser().parse_args([]).max_distance is None
    assert prealign._parser().parse_args(["--max-distance", "64"]).max_distance == 64
    assert prealign.TITLE == b"record\trepresentative\tstrand\tstart\tvotes\tmatches\n"


# ---- 2. the yardstick --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x,y,d", [(b"kitten", b"sitting", 3), (b"", b"ACGT", 4), (b"ACGT", b"ACGT", 0), (b"AAAA", b"AAAAA", 1),
                                   (b"ACGTACGT", b"CGTACGTA", 2), (b"N", b"N", 0), (b"a", b"A", 1), (b"", b"", 0), (b"\x00\xff", b"\xff\x00", 2)])
def test_answers_by_hand(x, y, d):
    assert D.lev(x, y) == d and D.lev(y, x) == d and D.table(x, y)[-1][-1] == d
    assert D.bounded(x, y, d) == d and (d == 0 or D.bounded(x, y, d - 1) == OVER)


def test_a_table_filled_by_hand():
    """GATCA (rows) against GTTACA (columns): 5 x 6 cells below and right of the border, filled by hand with the three rules."""
    #              ""  G  T  T  A  C  A
    by_hand = [[0, 1, 2, 3, 4, 5, 6],     # ""
               [1, 0, 1, 2, 3, 4, 5],     # G
               [2, 1, 1, 2, 2, 3, 4],     # A
               [3, 2, 1, 1, 2, 3, 4],     # T
               [4, 3, 2, 2, 2, 2, 3],     # C
               [5, 4, 3, 3, 2, 3, 2]]     # A
    assert D.table(b"GATCA", b"GTTACA") == by_hand
    for i in range(6):                                        # the numpy rows give the table's last column for every prefix
        assert D.lev(b"GATCA"[:i], b"GTTACA") == by_hand[i][6]
    for j in range(7):
        assert D.lev(b"GATCA", b"GTTACA"[:j]) == by_hand[5][j]


def test_the_rules_of_a_pair():
    seqs = [b"ACGTACGT", b"ACGAACGT", b"", b"ACG"]
    d, sc, within, bad = D.pairs(seqs, None, [(0, 1), (0, 0), (2, 3), (0, 3), (0, 4), (4, 0), (2, 2)], 3)
    assert d.tolist() == [1, 0, 3, OVER, OVER, OVER, 0] and (within, bad) == (4, 2)
    assert sc.tolist() == [[7, 8], [8, 8], [0, 3], [0, 8], [0, 0], [0, 0], [0, 0]]
    d, sc, within, bad = D.pairs(seqs, [b"ACGT", b""], [(3, 0), (3, 1), (1, 0)], 1, lengths_b=[4, 2 ** 31])
    assert d.tolist() == [1, OVER, OVER] and sc.tolist() == [[3, 4], [0, 0], [0, 8]] and (within, bad) == (1, 1)
    # identity 1 - d / L against a threshold in 2^-16: 7 / 8 links at 0.875 and not above
    assert D.links([[7, 8], [0, 8], [0, 0], [8, 8]], int(round(0.875 * 65536))).tolist() == [True, False, False, True]
    assert D.links([[7, 8]], int(round(0.875 * 65536)) + 1).tolist() == [False]


# ---- 3. the sets hold what they name ---------------------------------------------------------------------------------------------
def test_the_sets_hold_what_they_name():
    c = S.constants()
    cases = S.cases()
    assert c["SLICE_WORDS"] * 4 * c["DISTANCE_WAVES"] * 8 <= 160 * 1024        # eight workgroups a CU in 160 KiB of LDS
    assert 2 * S.row_words(c["DISTANCE_MAX"]) * 4 + c["STAGE_SLACK"] < c["SLICE_WORDS"] * 4
    # the staging limit: one below, at it, one above; and pairs on either path elsewhere
    sl = cases["stage_limit"]
    sums = [len(sl.a[i]) + len(sl.b[j]) for i, j in sl.pairs]
    assert sums[:3] == [S.stage_limit(sl.W) - 1, S.stage_limit(sl.W), S.stage_limit(sl.W) + 1]
    assert [S.staged(len(sl.a[i]), len(sl.b[j]), sl.W) for i, j in sl.pairs] == [True, True, False, False]
    assert max(len(s) for case in cases.values() for s in case.a + (case.b or [])) == S.stage_limit(sl.W)
    pg = cases["placement_global"]
    assert not any(S.staged(len(pg.a[i]), len(pg.b[j]), pg.W) for i, j in pg.pairs)
    for name in ("placement_tail", "placement_whole", "placement_global"):
        case = cases[name]
        assert case.off_a[0] != 0 and case.off_b[0] != 0 and len(case.pairs) == 64
        assert {(int(case.off_a[i]) % 8, int(case.off_b[j]) % 8) for i, j in case.pairs} == {(p, q) for p in range(8) for q in range(8)}
    # the cutoff: each W has a pair at it, one below and one above
    for W in (1, 8, 31, 32, 33, 63, 64):
        d = S.expected("cutoff_%d" % W)[0].tolist()
        assert d[:3] == [W - 1, W, OVER] and d[3:] == [W, OVER, W, OVER], W
    assert S.expected("cutoff_0")[0].tolist()[:3] == [0, 0, OVER]
    d = S.expected("cutoff_255")[0]
    assert (d == OVER).sum() >= 3 and ((d != OVER) & (d >= 200)).sum() >= 3 and d[-6:].tolist() == [255, OVER, OVER, 254, 255, OVER]
    assert S.expected("gap_unread")[0].tolist() == [OVER, OVER, 0, OVER]
    d = S.expected("repeats")[0].tolist()
    assert d[0] == 1 and d[1:7] == [1, 2, 2, 1, 2, 2] and all(0 < v <= 2 * k for k, v in zip(range(1, 6), d[7:12])) and d[12] == 2
    assert S.expected("bytes")[0].tolist()[:6] == [0, 4, 1, 0, 1, 2]
    assert S.expected("invalid")[3] == 5 and S.expected("too_long_a")[3] == 2 and S.expected("too_long_b")[3] == 3 and S.expected("no_records")[3] == 2
    assert S.expected("self_pairs")[0].tolist()[:6] == [0] * 6
    # the random set: 300 pairs, every cutoff of 0 .. 48 drawn from, a third within and a third over
    rnd = sorted(n for n in cases if n.startswith("random_"))
    d = np.concatenate([S.expected(n)[0] for n in rnd])
    assert len(d) == 300 and len(rnd) >= 40
    assert (d != OVER).sum() >= 100 and (d == OVER).sum() >= 100
    # one pair past the grid
    pg = S.past_the_grid()
    assert len(pg.pairs) == c["DISTANCE_MAX_GRID"] * c["DISTANCE_WAVES"] + 1


def test_the_planted_set_in_the_yardsticks():
    """Every copy, cut by the window the yardstick prealign finds, is within 64 of its founder: the distance is the full table's,
    and no more than the substitutions that were planted."""
    case, counts = S.planted()
    d, sc, within, bad = S.expected("planted")
    assert len(d) == 120 and within == 120 and bad == 0
    assert (d <= np.array(counts)).all() and (d > 0).all()
    for p in (0, 59, 119):
        i, j = case.pairs[p]
        assert D.table(case.a[i][:200], case.b[j][:200])[-1][-1] == D.lev(case.a[i][:200], case.b[j][:200])


# ---- 4. the routines as fibers -----------------------------------------------------------------------------------------------
def test_constants():
    from tests.emu import distance_emu
    c = S.constants()
    assert distance_emu.constants() == (c["DISTANCE_WAVES"], c["SLICE_WORDS"], c["STAGE_SLACK"], c["DISTANCE_MAX"])


def _check(name, got):
    dist, scores, within, invalid = S.expected(name)
    g_dist, g_scores, g_within, g_invalid = got
    if g_dist is not None:
        assert np.array_equal(g_dist, dist), (name, np.flatnonzero(g_dist != dist)[:8])
    if g_scores is not None:
        assert np.array_equal(g_scores, scores), name
    assert (g_within, g_invalid) == (within, invalid), name


def test_the_sets_as_fibers(tmp_path):
    """Every set but the one past the grid; three waves stride over the pairs, so a wave runs several pairs through one slice."""
    from tests.emu import distance_emu
    cases = S.cases()
    names = sorted(cases)
    assert {cases[n].out for n in names} == {"both", "distance", "scores"}
    got = distance_emu.run([cases[n] for n in names], tmp_path)
    for name, g in zip(names, got):
        _check(name, g)
    # one wave for all pairs, and more waves than pairs
    for waves in (1, 40):
        _check("lengths", distance_emu.run([cases["lengths"]], tmp_path, waves=waves)[0])


def test_the_planted_set_as_fibers(tmp_path):
    """All but the first five families (the fibers are slow; the card runs all)."""
    from tests.emu import distance_emu
    case, _ = S.planted()
    part = S.Case(case.a, case.b, case.W, case.pairs[15:])
    dist, scores, _, _ = S.expected("planted")
    g_dist, g_scores, within, invalid = distance_emu.run([part], tmp_path)[0]
    assert np.array_equal(g_dist, dist[15:]) and np.array_equal(g_scores, scores[15:]) and (within, invalid) == (105, 0)
