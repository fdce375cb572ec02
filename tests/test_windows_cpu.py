"""CPU-only: the windows surface of the ABI, the restatement tests/windows_ref.py against the pinned writers of rotate / cat /
decat / orfs, and the device routine circkit_amd/csrc/window_gather.h run as fibers by a stand-alone program
(tests/emu/windows_emu_main.cpp) against the restatement, byte for byte."""
import math
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import orfs_ref
from tests import windows_ref as R
from tests import windows_sets as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_examples")
NAMES = {"circkit_windows_gather_device": 9, "circkit_windows_status": 3, "circkit_windows_of_records_device": 7,
         "circkit_orfs_windows_device": 7, "circkit_windows_gather": 10}
ROTATE_FIXTURES = ("rotate_5", "rotate_minus_5", "rotate_0.25", "rotate_0.5")
PERCENTS = (0.5, 0.25, 0.999, 1.0, 1.5, -0.5, 1e30, -1e30, float("nan"))


def rotate_bases(n):
    return (1, -1, 3, -3, n, n + 1, -(n + 1), 2 ** 63 - 1, -2 ** 63)


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------
def test_the_surface():
    import __graft_entry__ as g
    g.build()
    import circkit_amd
    from circkit_amd import api
    from tests.test_abi import header_symbols
    lib = circkit_amd.load_library()
    syms = header_symbols()
    for name, n_args in NAMES.items():
        assert name in syms, "include/circkit.h does not declare %s" % name
        assert name in api.SIGNATURES and len(api.SIGNATURES[name][1]) == n_args, name
        assert hasattr(lib, name), "libcirckit_hip.so does not export %s" % name
    for method in ("windows_gather_device", "windows_status", "windows_of_records_device", "orfs_windows_device", "windows_gather"):
        assert callable(getattr(api.Context, method))
    for fn in ("rotate_batch", "cat_batch", "decat_batch", "revcomp_batch", "orf_sequences"):
        assert callable(getattr(circkit_amd, fn)) and callable(getattr(api.Context, fn))
    assert api.WINDOW_DTYPE.itemsize == 24 and api.WINDOW_DTYPE == R.WINDOW_DTYPE
    assert [api.WINDOW_KINDS[k] for k in ("rotate_bases", "rotate_percent", "cat", "decat", "revcomp")] == \
        [R.ROTATE_BASES, R.ROTATE_PERCENT, R.CAT, R.DECAT, R.REVCOMP]


# ---- 2. the restatement against the pinned writers ---------------------------------------------------------------------------
def packed_full_seqs(text):
    return S.pack_like(O.full_seq(raw) for _, raw in O.read_fasta(text))


def written_sequences(fasta):
    return [O.full_seq(raw) for _, raw in O.read_fasta(fasta)]


def expected_rotate(text, bases=None, percent=None):
    """oracle.cli_rotate's sequences.  It converts floor(n * percent) with Python's unbounded int(), src/rotate.rs:29 with
    `as i64`: where the product leaves the i64 range for every record (n >= 1, |percent| = 1e30) the saturated value goes in as
    --bases, which takes the same path from :37 on; NaN converts to 0, whose rotation index n writes the record unchanged."""
    if percent is not None and math.isnan(percent):
        return written_sequences(text)
    if percent is not None and abs(percent) >= 1e30:
        return written_sequences(O.cli_rotate(text, bases=R.I64_MAX if percent > 0 else R.I64_MIN))
    return written_sequences(O.cli_rotate(text, bases=bases, percent=percent))


def via_windows(data, offs, kind, **kw):
    out, out_off, bad = R.gather(data, offs, R.windows_of_records(np.diff(offs.astype(np.int64)), kind, **kw))
    assert bad == 0
    return S.split(out, out_off)


@pytest.mark.parametrize("name", ROTATE_FIXTURES + ("cat", "decat"))
def test_restatement_reproduces_rotate_cat_decat(name):
    text = open(os.path.join(GOLDEN, name, "in.fasta"), "rb").read()
    data, offs = packed_full_seqs(text)
    lengths = np.diff(offs.astype(np.int64))
    assert len(lengths) and lengths.min() > 0
    assert via_windows(data, offs, R.CAT) == written_sequences(O.cli_cat(text))
    assert via_windows(data, offs, R.DECAT) == written_sequences(O.cli_decat(text))
    for n in sorted(set(int(x) for x in lengths)):
        for b in rotate_bases(n):
            assert via_windows(data, offs, R.ROTATE_BASES, bases=b) == expected_rotate(text, bases=b), (name, b)
    for p in PERCENTS:
        assert via_windows(data, offs, R.ROTATE_PERCENT, percent=p) == expected_rotate(text, percent=p), (name, p)
    # the fixture's own flags give the fixture's own output
    flags = {"rotate_5": dict(bases=5), "rotate_minus_5": dict(bases=-5), "rotate_0.25": dict(percent=0.25), "rotate_0.5": dict(percent=0.5)}
    if name in flags:
        want = written_sequences(open(os.path.join(GOLDEN, name, "out.fasta"), "rb").read())
        kind = R.ROTATE_BASES if "bases" in flags[name] else R.ROTATE_PERCENT
        assert via_windows(data, offs, kind, **flags[name]) == want


def test_rotation_rules_at_the_edges():
    assert R.as_i64(float("nan")) == 0 and R.as_i64(1e30) == 2 ** 63 - 1 and R.as_i64(-1e30) == -2 ** 63 and R.as_i64(-0.0) == 0
    assert R.as_i64(2.0 ** 63) == 2 ** 63 - 1 and R.as_i64(-2.0 ** 63) == -2 ** 63 and R.as_i64(float("inf")) == 2 ** 63 - 1
    assert R.rotation_index(10, bases=-2 ** 63) == 2 ** 63 % 10 and R.rotation_index(10, bases=10) == 10
    w = R.windows_of_records([0, 7, 2 ** 32], R.ROTATE_BASES, bases=3)
    assert w.tolist() == [(0, 0, 0, 0, 0), (7, 1, 4, 0, 0), (2 ** 32, 2, 0, 0, 0)]
    assert R.windows_of_records([0, 7], R.CAT).tolist() == [(0, 0, 0, 0, 0), (14, 1, 0, 0, 0)]
    assert R.windows_of_records([0, 7], R.DECAT).tolist() == [(0, 0, 0, 0, 0), (3, 1, 0, 0, 0)]
    assert R.windows_of_records([0, 7], R.REVCOMP).tolist() == [(0, 0, 0, 1, 0), (7, 1, 0, 1, 0)]


ORF_FLAGS = (dict(), dict(max_wraps=3, no_stop_required=True, start_codons="ATG,CTG,TTG"))


@pytest.mark.parametrize("include_stop", (False, True))
@pytest.mark.parametrize("flags", ORF_FLAGS, ids=("default", "no-stop-required"))
def test_restatement_reproduces_the_orf_sequences(flags, include_stop):
    seqs = S.orf_records()
    data, offs = S.pack_like(seqs)
    want = S.sequence_lines(orfs_ref.cli_orfs(S.fasta_of(seqs), include_stop=include_stop, **flags)[0])
    kw = dict(start_codons=flags.get("start_codons", "ATG").split(","), min_length=75, max_wraps=flags.get("max_wraps", 3),
              require_stop=not flags.get("no_stop_required", False), strands=3, mode=0)
    orf_off, orfs = orfs_ref.orfs_batch(data, offs, **kw)
    out, out_off, bad = R.gather(data, offs, R.orf_windows(orf_off, orfs, include_stop))
    assert bad == 0 and len(want) > 100 and (orfs["strand"] == 1).any() and (orfs["length"] > np.diff(offs.astype(np.int64)).max()).any() == \
        bool(flags)
    assert S.split(out, out_off) == want


# ---- 3. the device routine on the CPU ----------------------------------------------------------------------------------------
def test_constants_move_the_boundary_cases():
    from tests.emu import windows_emu
    c = S.constants()
    assert windows_emu.constants() == (c["TILE_BYTES"], c["GATHER_WAVES"])
    shifted = dict(c, WSCAN_TILE=c["WSCAN_TILE"] * 2, TILE_BYTES=c["TILE_BYTES"] // 2)
    counts = lambda cc: sorted(len(w) for name, _, _, w, _ in S.boundary_cases(np.random.default_rng(0), cc))
    assert counts(shifted) != counts(c)
    assert {c["WSCAN_TILE"] - 1, c["WSCAN_TILE"], c["WSCAN_TILE"] + 1, c["TILE_BYTES"] // 16 - 1, c["TILE_BYTES"] // 16 + 1} <= set(counts(c))


def test_window_of_record_on_the_host():
    """The per-record rule of circkit_windows_of_records_device, compiled for the host with UBSan: every kind, the rotate grid,
    records of 0 symbols, at both sides of 2^32 and far beyond."""
    from tests.emu import windows_emu
    lengths = [0, 1, 2, 3, 999, 1000, 1001, 2_000_003, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 63, 2 ** 64 - 1]
    grid = [(R.ROTATE_BASES, dict(bases=b)) for n in (3, 1000, 2 ** 32 - 1) for b in rotate_bases(n)] + \
        [(R.ROTATE_PERCENT, dict(percent=p)) for p in PERCENTS + (-1.5, 1e-30, 4.3e9, -4.3e9, 2.0 ** 63, float("inf"), float("-inf"))] + \
        [(R.CAT, {}), (R.DECAT, {}), (R.REVCOMP, {})]
    for kind, kw in grid:
        assert np.array_equal(windows_emu.of_records(lengths, kind, **kw), R.windows_of_records(lengths, kind, **kw)), (kind, kw)


def test_saturated_rotations_by_hand():
    """The saturating conversions, independent of the restatement's own rule: rotations worked out by hand from src/rotate.rs.
    `floor(n * 1e30) as i64` is i64::MAX = 9223372036854775807 and `floor(n * -1e30) as i64` is i64::MIN, |i64::MIN| = 2^63 =
    9223372036854775808; NaN `as i64` is 0.  n = 10: MAX mod 10 = 7, idx = 10 - 7 = 3; 2^63 mod 10 = 8, idx = 8.  n = 7:
    2^63 = 8^21 = 1 mod 7, so MAX mod 7 = 0, idx = 7, the record as it is; 2^63 mod 7 = 1, idx = 1.  s = 0: idx = n, the record
    as it is.  The written record is seq[idx..] + seq[..idx]."""
    from tests.emu import windows_emu
    seqs = [b"ACGTTGCAAG", b"GATTACA"]
    by_hand = {1e30: ([3, 0], [b"TTGCAAGACG", b"GATTACA"]), -1e30: ([8, 1], [b"AGACGTTGCA", b"ATTACAG"]),
               float("nan"): ([0, 0], [b"ACGTTGCAAG", b"GATTACA"])}
    data, offs = S.pack_like(seqs)
    for p, (starts, written) in by_hand.items():
        assert via_windows(data, offs, R.ROTATE_PERCENT, percent=p) == written, p
        for w in (R.windows_of_records([10, 7], R.ROTATE_PERCENT, percent=p), windows_emu.of_records([10, 7], R.ROTATE_PERCENT, percent=p)):
            assert w["start"].tolist() == starts and w["length"].tolist() == [10, 7] and not w["strand"].any(), p
    for b, starts in ((2 ** 63 - 1, [3, 0]), (-2 ** 63, [8, 1])):
        assert windows_emu.of_records([10, 7], R.ROTATE_BASES, bases=b)["start"].tolist() == starts, b


def test_device_routine_as_fibers(tmp_path):
    """Every case of tests/windows_sets.py through effective_length + gather_tile in one child process; the program checks its
    canaries, that the payload and the windows are unchanged and that the lanes of each wave agree on their first window."""
    from tests.emu import windows_emu
    cases = S.all_cases()
    assert {p.get("in_shift", 0) for *_, p in cases} == set(range(16)) == {p.get("out_shift", 0) for *_, p in cases}
    got = windows_emu.run([(d, o, w, p) for _, d, o, w, p in cases], tmp_path)
    for (name, data, offs, wins, _), (out, out_off, total, bad) in zip(cases, got):
        exp, exp_off, exp_bad = R.gather(data, offs, wins)
        assert np.array_equal(out_off, exp_off), name
        assert total == len(exp) and bad == exp_bad, name
        assert np.array_equal(out, exp), name
    grid = R.gather(*cases[0][1:4])
    assert grid[2] > 10 and len(grid[0]) > 100_000


def test_fibers_refuse_a_short_capacity(tmp_path):
    from tests.emu import windows_emu
    name, data, offs, wins, _ = S.shift_cases(np.random.default_rng(3))[5]
    exp, exp_off, _ = R.gather(data, offs, wins)
    got = windows_emu.run([(data, offs, wins, dict(capacity=len(exp) - 1)), (data, offs, wins, dict(capacity=0)),
                           (data, offs, wins, dict(capacity=len(exp)))], tmp_path)
    for out, out_off, total, _ in got[:2]:
        assert out is None and total == len(exp) and np.array_equal(out_off, exp_off)      # (the program found every byte still canary)
    assert np.array_equal(got[2][0], exp)


def test_a_payload_across_byte_2_32_as_fibers(tmp_path):
    """The grid case and the window across tiles with the payload 2^32 bytes, less half a record, into a lazily reserved buffer
    (tests/high_base.py, "middle"): the 100-symbol record straddles byte 2^32 of the buffer, the 1000-symbol record lies wholly above
    it, and payload positions need 33 bits."""
    from tests import high_base as H
    from tests.emu import windows_emu
    cases = [S.all_cases()[0], S.all_cases()[-1]]
    assert cases[1][0] == "a window across tiles"
    leads = [int(H.conditions(data, offs, H.inner_longest(offs), "middle")[0]) for _, data, offs, _, _ in cases]
    got = windows_emu.run([(d, o, w, dict(p, lead=lead)) for (_, d, o, w, p), lead in zip(cases, leads)], tmp_path)
    for (name, data, offs, wins, _), (out, out_off, total, bad) in zip(cases, got):
        exp, exp_off, exp_bad = R.gather(data, offs, wins)
        assert np.array_equal(out_off, exp_off) and total == len(exp) and bad == exp_bad, name
        assert np.array_equal(out, exp), name
