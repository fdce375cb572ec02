"""The monomer compact (circkit_amd/csrc/monomer_compact.h) run on the CPU: decide() as one lane runs it and the gather's
workgroup body as 64 fibers per wave with the product's wave count (tests/emu/compact_emu.cpp: UBSan + bounds checks, a lane
that skips a collective deadlocks and is reported), against the restatement tests/monomers_ref.py.  The loader puts canaries
round the payload and every output, checks that the input is unchanged and that the lanes of a wave agree on the record
their search found."""
import numpy as np
import pytest

from tests import monomers_ref as MR
from tests import monomers_sets as MS
from tests.emu import compact_emu as E


def check(case, **place):
    name, data, offs, ends, full_len, flt = case
    exp = MR.compact(data, offs, ends, full_len, **flt)
    got = E.compact(data, offs, ends, full_len, **place, **flt)
    MR.assert_equal(got, exp, (name, place))
    return exp


def test_geometry_matches_the_named_constants():
    c = MS.constants()
    assert E.tile_bytes() == c["TILE_BYTES"] and E.waves() == c["GATHER_WAVES"]
    assert c["TILE_BYTES"] % 16 == 0


def test_emulator_sets():
    sets = MS.emulator_sets(E.tile_bytes())
    names = [s[0] for s in sets]
    assert len(set(names)) == len(names)
    written = 0
    for s in sets:
        written += len(check(s)[0])
    assert written > 4 * E.tile_bytes()


def test_emulator_sets_shifted():
    """The same sets with the payload and the output at odd addresses and offsets[0] != 0: tile and record boundaries fall
    elsewhere in the records."""
    for k, s in enumerate(MS.emulator_sets(E.tile_bytes())):
        check(s, in_shift=(3 * k + 1) % 16, out_shift=(5 * k + 7) % 16, lead=(7 * k) % 37)


def test_every_misalignment_pair():
    s = MS.misalignment_set()
    for i in range(16):
        for o in range(16):
            check(s, in_shift=i, out_shift=o, lead=(i + 3 * o) % 19)


def test_tile_boundary_on_a_record_boundary_at_every_output_shift():
    """With the output at shift a the first tile ends at output byte TILE - a: a record boundary there and one byte either side."""
    rng = np.random.default_rng(5)
    T = E.tile_bytes()
    for a in (0, 1, 8, 15):
        for d in (-1, 0, 1):
            first = T - a + d
            check(MS.case("tile end", rng, [first, 3, 0, 70], [first, 3, 0, 70]), out_shift=a, in_shift=(a + 5) % 16)


def test_filters_at_their_boundaries():
    for name, lengths, ends, full_len, flt, kept in MS.filter_boundary_cases():
        rng = np.random.default_rng(1)
        data, offs = MS.batch(rng, lengths)
        case = (name, data, offs, np.array(ends, dtype=np.uint32), np.array(full_len, dtype=np.uint64), flt)
        exp = check(case)
        slow = MR.compact_slow(data, offs, case[3], case[4], **flt)
        MR.assert_equal(exp, slow, name)
        assert (int(exp[3][0]) != MR.NONE) == kept, name
        check((name, data, offs, case[3], case[4], dict(flt, keep_all=True)))


def test_decide_on_random_triples_equals_the_plain_restatement():
    rng = np.random.default_rng(12)
    n = 4000
    lengths = rng.integers(0, 40, size=n)
    ends = rng.integers(0, 45, size=n).astype(np.uint32)
    ends[rng.random(n) < 0.2] = MR.NONE
    full = lengths + rng.integers(0, 5, size=n)
    data, offs = MS.batch(rng, lengths, b"ACGT")
    for flt in (dict(), dict(keep_all=True), dict(min_length=10, max_length=30), dict(min_overlap=7), dict(min_overlap_percent=0.51),
                dict(min_overlap_percent=1.0, keep_all=True), dict(min_length=3, min_overlap=2, min_overlap_percent=0.25, max_length=38)):
        exp = check(("random", data, offs, ends, full, flt))
        MR.assert_equal(exp, MR.compact_slow(data, offs, ends, full, **flt), flt)


def test_a_payload_across_byte_2_32():
    """The payload 2^32 bytes, less half a record, into a lazily reserved buffer (tests/high_base.py, "middle"): the longest record
    straddles byte 2^32 of the buffer, the records behind it lie wholly above, and payload positions need 33 bits."""
    from tests import high_base as H
    ran = 0
    for s in (MS.misalignment_set(), MS.emulator_sets(E.tile_bytes())[0], MS.emulator_sets(E.tile_bytes())[13]):
        j = H.inner_longest(s[2])
        absolute = H.conditions(s[1], s[2], j, "middle")
        check(s, in_shift=5, out_shift=11, lead=int(absolute[0]))
        ran += 1
    assert ran == 3 and MS.emulator_sets(E.tile_bytes())[13][0] == "a monomer across tiles"
