"""CPU-only: the cluster surface of the ABI, the yardstick tests/cluster_ref.py against hand-worked answers of the definition, the
condition on the planted families, and the device routines of circkit_amd/csrc/cluster.h run as fibers by a stand-alone program
(tests/emu/cluster_emu_main.cpp) against the yardstick: every key, offset, pair, label and total."""
import ctypes

import numpy as np
import pytest

from tests import cluster_ref as C
from tests import cluster_sets as S
from tests import sketch_ref as R

NAMES = {"circkit_cluster_candidates_device": 8, "circkit_cluster_candidates_status": 2, "circkit_cluster_link_device": 7,
         "circkit_cluster_link_status": 4, "circkit_cluster_batch": 8}
INVALID_ARG = -1


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
    for method in ("cluster_candidates_device", "cluster_candidates_status", "cluster_link_device", "cluster_link_status", "cluster_batch"):
        assert callable(getattr(api.Context, method))
    for fn in ("cluster_params", "cluster_batch"):
        assert callable(getattr(circkit_amd, fn))
    assert callable(circkit_amd.cluster.cluster_fasta)
    assert ctypes.sizeof(api.ClusterParams) == 24
    p = circkit_amd.cluster_params()
    assert (p.n_bands, p.band_bins, p.min_similarity_q16, p.min_filled, tuple(p.reserved)) == (64, 2, 13107, 8, (0, 0))
    p = circkit_amd.cluster_params(n_bands=1, band_bins=16, min_similarity=1.0, min_filled=1)
    assert (p.n_bands, p.band_bins, p.min_similarity_q16, p.min_filled) == (1, 16, 65536, 1)
    header = open(os.path.join(ROOT, "include", "circkit.h")).read()
    assert re.search(r"uint32_t n_bands;.*?uint32_t band_bins;.*?uint32_t min_similarity_q16;.*?uint32_t min_filled;.*?uint32_t reserved\[2\];.*?"
                     r"\} circkit_cluster_params;", header, flags=re.S)


def test_a_null_ctx_is_refused_without_a_device():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    lib = circkit_amd.load_library()
    p = circkit_amd.cluster_params()
    sp = circkit_amd.sketch_params()
    t = ctypes.c_uint64(7)
    assert lib.circkit_cluster_candidates_device(None, None, 0, 8, ctypes.byref(p), None, None, 0) == INVALID_ARG
    assert lib.circkit_cluster_candidates_status(None, ctypes.byref(t)) == INVALID_ARG
    assert lib.circkit_cluster_link_device(None, 0, None, None, 0, ctypes.byref(p), None) == INVALID_ARG
    assert lib.circkit_cluster_link_status(None, ctypes.byref(t), None, None) == INVALID_ARG
    assert lib.circkit_cluster_batch(None, None, None, 0, ctypes.byref(sp), ctypes.byref(p), None, ctypes.byref(t)) == INVALID_ARG
    assert t.value == 7


def test_the_command_line_without_a_device(tmp_path):
    from circkit_amd import cluster
    a = cluster._parser().parse_args([])
    assert (a.input, a.output, a.k, a.bins, a.bands, a.band_bins, a.min_similarity, a.table) == (None, None, 21, 256, 64, 2, 0.2, None)
    a = cluster._parser().parse_args(["-i", "in.fa", "-o", "out.fa", "--k", "15", "--bins", "64", "--bands", "16", "--band-bins", "4",
                                      "--min-similarity", "0.5", "--table", "t.tsv"])
    assert (a.input, a.output, a.k, a.bins, a.bands, a.band_bins, a.min_similarity, a.table) == ("in.fa", "out.fa", 15, 64, 16, 4, 0.5, "t.tsv")
    for bins in ("100", "0"):
        with pytest.raises(SystemExit) as e:
            cluster.main(["--bins", bins])
        assert e.value.code == 2
    assert cluster.main(["-i", str(tmp_path / "missing.fasta")]) == 1
    assert cluster._word(b"rec7 some words") == b"rec7" and cluster._word(b"") == b"" and cluster._word(b"one") == b"one"


# ---- 2. the yardstick --------------------------------------------------------------------------------------------------------
E = R.EMPTY
SIX_ROWS = [[10, 20, 30], [11, 20, 31], [10, 20, 32], [12, E, 31], [12, 21, 30], [13, 22, 33]]
SIX_OFFSETS = [0, 0, 1, 2, 3, 5, 5]
SIX_PAIRS = [(0, 1), (0, 2), (1, 3), (3, 4), (0, 4)]
#   record 1: band 1 with record 0.  record 2: bands 0 and 1 with record 0, once.  record 3: band 1 has no key, band 2 with record
#   1.  record 4: band 0 with record 3, then band 2 with record 0, in band order.  record 5: nothing.


def test_band_key_spelled_out():
    golden = 0x9e3779b97f4a7c15
    for b, v in ((0, 5), (1, 5), (63, 2 ** 64 - 2), (7, 0)):
        x = ((b + 1) * golden) % 2 ** 64
        assert C.band_key([None] * b + [v], b, 1) == R.fmix64(x ^ v)
    # two bins: the second is mixed into the first's result; the band index, not the bins' position in the row, seeds the key
    assert C.band_key([3, 4], 0, 2) == R.fmix64(R.fmix64(golden ^ 3) ^ 4)
    assert C.band_key([0, 0, 3, 4], 1, 2) == R.fmix64(R.fmix64(((2 * golden) % 2 ** 64) ^ 3) ^ 4) != C.band_key([3, 4], 0, 2)
    assert C.band_key([3, E], 0, 2) is None and C.band_key([E, 3], 0, 2) is None and C.band_key([E], 0, 1) is None
    assert C.band_key([S.key_of_none([], 4)] * 5, 4, 1) is None
    v = S.key_of_none([17], 2)
    assert C.band_key([0, 0, 0, 0, 17, v], 2, 2) is None and C.band_key([0, 0, 0, 0, 17, v ^ 1], 2, 2) is not None


def test_six_records_by_hand():
    assert C.candidates(SIX_ROWS, 3, 1) == (SIX_OFFSETS, SIX_PAIRS)
    scores = [(10, 10), (1, 100), (10, 10), (10, 10), (1, 100)]
    assert C.link(6, SIX_PAIRS, scores, S.DEFAULT) == ([0, 0, 2, 0, 0, 5], 3, 3, 0)
    # the order of the pairs and their orientation do not reach the labels
    back = [(j, i) for i, j in reversed(SIX_PAIRS)]
    assert C.link(6, back, list(reversed(scores)), S.DEFAULT) == ([0, 0, 2, 0, 0, 5], 3, 3, 0)
    assert C.link(6, SIX_PAIRS, [(10, 10)] * 5, S.DEFAULT) == ([0, 0, 0, 0, 0, 5], 2, 5, 0)
    assert C.link(6, SIX_PAIRS + [(6, 0), (2, 2)], [(10, 10)] * 7, S.DEFAULT) == ([0, 0, 0, 0, 0, 5], 2, 5, 1)


def test_the_threshold_by_hand():
    assert C.links(25, 100, 16384, 8) and not C.links(24, 100, 16384, 8)
    assert C.links(20, 100, 13107, 8) and not C.links(19, 100, 13107, 8)
    assert not C.links(7, 7, 0, 8) and C.links(0, 8, 0, 8) and not C.links(0, 0, 0, 1)
    assert C.links(8, 8, 65536, 8) and not C.links(1023, 1024, 65536, 8)
    assert C.q16(0.2) == 13107 and C.q16(1.0) == 65536 and C.q16(0.0) == 0


def test_the_sets_hold_what_they_name():
    exp = {name: S.expected_candidates(name) for name in S.candidate_cases()}
    for name in ("shared_8x2", "shared_64x1", "shared_5x3"):
        nb = S.candidate_cases()[name][1]
        assert exp[name][1].tolist() == [[0, r] for r in range(1, nb + 1)], name
    assert exp["empty_beside_equal"][1].tolist() == [[0, 1]]
    assert exp["all_empty_rows"][1].tolist() == [[2, 6]]
    assert exp["no_key_1bin"][1].tolist() == [[0, 4]] and exp["no_key_2bins"][1].tolist() == [[0, 4]]
    assert exp["several_earlier"][1].tolist() == [[0, 1], [0, 3], [2, 5], [0, 5], [4, 5], [3, 6], [5, 6]]
    assert exp["identical_x1000"][1].tolist() == [[0, i] for i in range(1, 1000)]
    assert exp["records_0"][0].tolist() == [0] and exp["records_1"][0].tolist() == [0, 0]
    for name, (offsets, pairs) in exp.items():
        assert len(pairs) == offsets[-1] and (name.startswith("records_") and name[8:] in "01" or len(pairs)), name
        assert (pairs[:, 0] < pairs[:, 1]).all()
    for name in S.link_cases():
        S.expected_link(name)
    assert S.expected_link("invalid_among_valid")[1:] == (2, 3, 5)
    assert S.expected_link("self_pairs")[1:] == (4, 1, 0)
    assert S.expected_link("ratio_one_below")[0].tolist() == [0, 1, 2, 2] and S.expected_link("ratio_0.2")[0].tolist() == [0, 1, 2, 2]
    assert S.expected_link("filled_below_min")[0].tolist() == [0, 1, 2, 2] and S.expected_link("zero_zero")[0].tolist() == [0, 1, 2, 2]
    assert S.expected_link("threshold_0")[0].tolist() == [0, 0, 2, 3, 4, 4] and S.expected_link("threshold_65536")[0].tolist() == [0, 0, 2, 3, 4, 4]
    assert S.expected_link("duplicate_rejected_once")[0].tolist() == [0, 0, 2, 3]
    for name, clusters in (("star", 3), ("path", 1), ("clique", 3), ("two_joined_last", 1), ("many_components", 40)):
        assert S.expected_link(name, True)[1] == clusters, name


def test_the_planted_families_in_the_yardstick():
    """The condition on the inputs, with the yardstick alone: every record's label is the smallest index of its planted family, no
    candidate joins two families, and the threshold is read."""
    records, family = S.families()
    rows, offsets, pairs, scores, labels, n_clusters, n_linked = S.families_expected()
    assert len(records) == 240 and len(set(family)) == 120
    fam = np.array(family)
    assert (fam[pairs[:, 0]] == fam[pairs[:, 1]]).all(), "a candidate joins two families"
    assert np.array_equal(labels, S.family_labels(family)) and n_clusters == 120
    assert (scores[:, 0] / scores[:, 1]).min() >= 0.2 and n_linked == len(pairs)
    assert S.families_expected(0.9)[5] > 120


# ---- 3. the device routines on the CPU ---------------------------------------------------------------------------------------
def test_constants():
    from tests.emu import cluster_emu
    c = S.constants()
    assert cluster_emu.constants() == (c["SCAN_WG"], c["SCAN_ITEMS"])
    assert len(S.past_the_emit_grid()[0]) == c["EMIT_MAX_GRID"] * c["EMIT_WAVES"] + 1


def keys_of(rows, nb, bb):
    return np.array([[C.NO_KEY if (k := C.band_key([int(v) for v in row], b, bb)) is None else k for b in range(nb)] for row in rows],
                    dtype=np.uint64).reshape(len(rows), nb)


def test_candidates_as_fibers(tmp_path):
    """Every set; the waves of either kernel on both sides of the work; a capacity that just holds everything."""
    from tests.emu import cluster_emu
    names = list(S.candidate_cases())
    cases = []
    for i, name in enumerate(names):
        rows, nb, bb = S.candidate_cases()[name]
        cases.append((rows, nb, bb, len(rows) * nb, (1, 3, 40)[i % 3], (1, 5, 70)[i % 3]))
    got = cluster_emu.run_candidates(cases, tmp_path)
    for name, case, (keys, offsets, pairs, total) in zip(names, cases, got):
        rows, nb, bb, cap = case[:4]
        exp_off, exp_pairs = S.expected_candidates(name)
        assert np.array_equal(keys, keys_of(rows, nb, bb)), name
        assert np.array_equal(offsets, exp_off) and total == len(exp_pairs), name
        assert np.array_equal(pairs, S.pair_buffer(exp_off, exp_pairs, cap, cluster_emu.UNWRITTEN)), name


def test_capacity_as_fibers(tmp_path):
    from tests.emu import cluster_emu
    rows, nb, bb = S.candidate_cases()["several_earlier"]
    exp_off, exp_pairs = S.expected_candidates("several_earlier")
    total = len(exp_pairs)
    caps = [total, total - 1, total // 2, 1, 0]
    got = cluster_emu.run_candidates([(rows, nb, bb, cap, 2, 2) for cap in caps], tmp_path)
    for cap, (keys, offsets, pairs, t) in zip(caps, got):
        assert np.array_equal(offsets, exp_off) and t == total, cap
        assert np.array_equal(pairs, S.pair_buffer(exp_off, exp_pairs, cap, cluster_emu.UNWRITTEN)), cap
    # what the rule means on this set: one pair short, the last record's two pairs are missing and nobody else's
    assert (got[1][2][:total - 2] == exp_pairs[:total - 2]).all() and (got[1][2][total - 2:] == cluster_emu.UNWRITTEN).all()


def test_one_record_past_the_emit_grid_as_fibers(tmp_path):
    """The large set on a small grid of fibers: every wave makes many trips."""
    from tests.emu import cluster_emu
    rows, nb, bb = S.past_the_emit_grid()
    rows = rows[:600]
    offsets, pairs = C.candidates([[int(v) for v in row] for row in rows], nb, bb)
    keys, got_off, got_pairs, total = cluster_emu.run_candidates([(rows, nb, bb, len(pairs), 16, 16)], tmp_path)[0]
    assert total == len(pairs) > 300 and got_off.tolist() == offsets and got_pairs.tolist() == [list(p) for p in pairs]


def test_link_as_fibers(tmp_path):
    from tests.emu import cluster_emu
    names = list(S.link_cases())
    cases = [(*S.link_cases()[name], (1, 2, 9)[i % 3], (1, 3)[i % 2]) for i, name in enumerate(names)]
    small = [(*S.contention(name, True), 4, 4) for name in S.CONTENTION]
    got = cluster_emu.run_link(cases + small, tmp_path)
    for name, (labels, clusters, linked, invalid) in zip(names + list(S.CONTENTION), got):
        exp = S.expected_link(name, name in S.CONTENTION)
        assert np.array_equal(labels, exp[0]) and (clusters, linked, invalid) == exp[1:], name


def test_the_planted_families_as_fibers(tmp_path):
    from tests.emu import cluster_emu
    rows, offsets, pairs, scores, labels, n_clusters, n_linked = S.families_expected()
    p = S.FAMILY_PARAMS
    keys, got_off, got_pairs, total = cluster_emu.run_candidates([(rows, p["n_bands"], p["band_bins"], len(rows) * p["n_bands"], 8, 8)], tmp_path)[0]
    assert np.array_equal(got_off, offsets) and np.array_equal(got_pairs[:total], pairs) and total == len(pairs)
    for sim in (0.2, 0.9):
        exp = S.families_expected(sim)
        got = cluster_emu.run_link([(len(rows), pairs, scores, (C.q16(sim), p["min_filled"]), 3, 2)], tmp_path)[0]
        assert np.array_equal(got[0], exp[4]) and got[1:] == (exp[5], exp[6], 0)
