"""The inputs of tests/test_high_base_gpu.py, checked without a GPU: every set of its Part A, in every placement, has a record
wholly below byte 2^32 of the payload buffer, one wholly above, record j placed as asked, fits the 8 MiB window round the line,
and reads a different byte from the alias region at every position above the line -- so that a payload position truncated to 32
bits is a definite wrong answer and not an accident."""
import numpy as np
import pytest

from tests import high_base as H

SETS = H.sets()


def test_place_by_hand():
    offs = np.array([0, 10, 10, 17, 30], dtype=np.uint64)
    a = H.place(offs, 2, "middle")
    assert a.dtype == np.uint64 and a.tolist() == [H.LINE - 13, H.LINE - 3, H.LINE - 3, H.LINE + 4, H.LINE + 17]
    b = H.place(offs, 3, "boundary")
    assert b.tolist() == [H.LINE - 17, H.LINE - 7, H.LINE - 7, H.LINE, H.LINE + 13] and int(b[3]) & 0xFFFFFFFF == 0
    assert H.place(offs, 3, "boundary", at=5)[3] == H.LINE - 5
    assert H.place(offs + np.uint64(7), 2, "middle").tolist() == a.tolist()              # (offsets[0] != 0 goes into the lead)
    with pytest.raises(AssertionError):
        H.place(offs, 1, "middle")                                                      # an empty record has no middle
    with pytest.raises(AssertionError):
        H.place(np.array([0, H.HALF + 2, 2 * H.HALF + 4], dtype=np.uint64), 0, "boundary")   # beyond the window
    assert H.inner_longest(offs) == 2 and H.inner_longest(np.array([0, 5, 9], dtype=np.uint64)) is None


def test_decoy_and_its_alias():
    d = H.decoy(3, 1000)
    assert np.array_equal(d, H.decoy(3, 1000)) and not np.array_equal(d, H.decoy(4, 1000)) and set(d.tolist()) == set(b"ACGT")
    data = np.concatenate([d[500:600], d[:200]])                                        # above the line: equal to its alias at every byte
    absolute = np.array([H.LINE - 100, H.LINE, H.LINE + 200], dtype=np.uint64)
    e = H.differing(d, data, absolute)
    assert (e[:200] != data[100:]).all() and np.array_equal(e[200:], d[200:]) and set(e.tolist()) <= set(b"ACGT")
    assert np.array_equal(H.differing(d, data, absolute - np.uint64(500)), d)           # nothing above the line: unchanged


def test_the_list_names_every_unit_in_both_modes():
    names = {s[0].split()[0] for s in SETS}
    assert names == {"sketch", "monomerize", "monomers", "uniq", "windows", "translate", "fasta", "canon"}
    for unit in names:
        assert {s[4] for s in SETS if s[0].split()[0] == unit} == set(H.MODES), unit
    # the cases of the monomer compact that have no "middle": their longest record has fewer than 2 bytes
    no_middle = sorted(c[0] for c, j in H.monomers_cases() if j is None)
    assert no_middle == sorted(H.NO_MIDDLE)
    assert all(s[3] is not None for s in SETS)


@pytest.mark.parametrize("k", range(len(SETS)), ids=["%s-%s%s" % (s[0].replace(" ", "_"), s[4], "+%d" % s[5] if s[5] else "") for s in SETS])
def test_conditions(k):
    name, data, offs, j, mode, at = SETS[k]
    H.conditions(data, offs, j, mode, at)


def test_the_extra_sketch_record_and_the_dimer():
    for kind in ("lengths", "symbols"):
        for k, _ in H.SKETCH_PARAMS:
            recs, j, seg = H.sketch_records(kind, k)
            assert len(recs[j]) == 3 * seg + 500 == max(len(r) for r in recs)
            o = H.place(H.pack(recs)[1], j, "middle").astype(np.int64)
            assert seg < H.LINE - o[j] < 2 * seg                                        # the line inside the second span
            assert H.place(H.pack(recs)[1], j, "boundary", seg)[j] + np.uint64(seg) == H.LINE
    recs, j = H.mono_records()
    assert len(recs[j]) == 2200 and recs[j][1100:] != recs[j][:1100] and sum(a != b for a, b in zip(recs[j][:1100], recs[j][1100:])) == 1
    o = H.place(H.pack(recs)[1], j, "middle").astype(np.int64)
    assert o[j] + 1100 == H.LINE                                                        # the second copy starts on the line


def test_canon_and_uniq_sets():
    sets = H.canon_sets()
    assert sorted(len(s) for s in sets["every_length"]) == list(range(2101)) and set(H.CANON_CRAFTED) < set(sets)
    for name, data, offs, fs, base, j in H.uniq_cases():
        own = np.uint64(base) + np.arange(H.UNIQ_COUNT, dtype=np.uint64)
        kept = fs == own
        assert 0.2 < kept.mean() < 0.95 and len(offs) == H.UNIQ_COUNT + 1
        if base:
            assert (fs[~kept] > 2 ** 32).any() and (fs[~kept] < base).any()


def test_the_blocks_put_the_line_where_the_tests_say():
    """Byte 2^32 inside a sequence line, inside a header, and on a '>' that
    directly follows a '\\n'; and the host parse of three blocks in a row is the arithmetic tests/test_past_4gib_gpu.py uses."""
    from tests import fasta_sets as F
    for where in ("sequence", "header", "record start"):
        b = H.block_for(where)
        at = H.LINE % len(b)
        if where == "record start":
            assert b[at - 1:at + 1] == b"\n>"
        elif where == "header":
            line = b[b.rfind(b"\n", 0, at) + 1:b.find(b"\n", at)]
            assert line.startswith(b">") and b[at:at + 1] != b"\n"
        else:
            line = b[b.rfind(b"\n", 0, at) + 1:b.find(b"\n", at)]
            assert not line.startswith(b">") and len(line.strip()) > 2 and b[at:at + 1] not in b"\r\n"
        one, three = F.host(b), F.host(b * 3)
        r, P = one["records"], len(one["data"])
        assert r == 5 and one["consumed"] == len(b) and three["records"] == 3 * r and three["consumed"] == 3 * len(b)
        assert np.array_equal(three["data"], np.tile(one["data"], 3))
        for i in range(3):
            assert np.array_equal(three["offsets"][i * r:(i + 1) * r], one["offsets"][:r] + np.uint64(i * P))
            for key in ("head", "raw"):
                assert np.array_equal(three[key][i * r:(i + 1) * r], one[key] + np.array([i * len(b), 0], dtype=np.uint64))
