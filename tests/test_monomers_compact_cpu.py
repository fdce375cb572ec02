"""CPU-only checks behind the monomer compact: the restatement the GPU is compared with (tests/monomers_ref.py) against the
writer that is pinned to the reference's fixtures (tests/mono_ref.py), the claim that the worker's pre-check needs no step
of its own, the scan's edge list rederived from the kernel's constants, and the Python surface of the new entry points."""
import ctypes
import os

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S
from tests import monomers_ref as MR
from tests import monomers_sets as MS

# The record counts of tests/test_monomers_compact_gpu.py test_scan_edges: both sides of a workgroup of the decide kernel
# (COMPACT_WG), of a scan tile (CSCAN_TILE records), of one round of CSCAN_WG tile sums in the single-workgroup second level
# (CSCAN_CHUNK), and one count in a third round
SCAN_COUNTS = [1, 255, 256, 257, 2047, 2048, 2049, 524_287, 524_288, 524_289, 1_048_577]


def test_scan_counts_straddle_the_kernel_edges():
    """If a launch constant of the compact's kernels changes, SCAN_COUNTS above must move with it."""
    c = MS.constants()
    for name in ("COMPACT_WG", "CSCAN_TILE", "CSCAN_CHUNK"):
        edge = c[name]
        assert {edge - 1, edge, edge + 1} <= set(SCAN_COUNTS), ("SCAN_COUNTS", name, edge)
    assert 1 in SCAN_COUNTS and 2 * c["CSCAN_CHUNK"] < max(SCAN_COUNTS) <= 2 * c["CSCAN_CHUNK"] + c["CSCAN_TILE"], "a third round"


# ---- the restatement against the pinned writer ---------------------------------------------------------------------------
def compact_of_fasta(text, sensitive=False, seed_length=10, max_mismatch=None, min_identity=None, **flt):
    """The compact of a FASTA text as the device sees it: the normalized records, full_seq().len() per record, the end
    indices of the restated Monomerizer WITHOUT the worker's pre-check.  Returns (records, norms, result of MR.compact)."""
    from oracle import oracle as O
    recs = [(h, O.full_seq(raw), O.normalize(raw)[0]) for h, raw in O.read_fasta(text)]
    data, offs = S.pack([r[2] for r in recs])
    ends = R.batch(data, offs, threads=2, seed_len=seed_length, max_mismatch=max_mismatch, min_identity=min_identity, sensitive=sensitive)
    full_len = np.array([len(r[1]) for r in recs], dtype=np.uint64)
    res = MR.compact(data, offs, ends, full_len, **flt)
    MR.assert_equal(res, MR.compact_slow(data, offs, ends, full_len, **flt), "vectorized against plain")
    return recs, res


def against_the_writer(text, **flags):
    from oracle import oracle as O
    fasta, table = R.cli_monomerize(text, table_delim=b"\t", **flags)
    recs, (out, out_off, out_src, kept) = compact_of_fasta(text, **flags)
    written = O.read_fasta(fasta)
    rows = [l.rsplit(b"\t", 2) for l in table.split(b"\n")[1:] if l] if table else []
    assert [h for h, _ in written] == [recs[int(i)][0] for i in out_src], "another set of records is written"
    assert len(rows) == len(written)
    compared = 0
    for j, ((head, seq), row) in enumerate(zip(written, rows)):
        i = int(out_src[j])
        _, full, norm = recs[i]
        mine = int(out_off[j + 1] - out_off[j])
        if int(kept[i]) != MR.NONE:
            assert mine == int(kept[i]) == len(seq) == int(row[2]), (head, mine, len(seq), row)
        else:                                   # keep_all: the reference writes full_seq whole, the compact the normalized record whole
            assert flags.get("keep_all") and len(seq) == len(full) == int(row[2]) and mine == len(norm), head
        assert int(row[1]) == len(full)
        if len(full) == len(norm):
            assert O.normalize(seq)[0] == bytes(out[int(out_off[j]):int(out_off[j + 1])]), head
            compared += 1
    return len(written), compared


@pytest.mark.parametrize("name", sorted(S.FIXTURES))
def test_restatement_on_the_cli_fixtures(name):
    text = open(os.path.join(S.EXAMPLES, name, "in.fasta"), "rb").read()
    n, compared = against_the_writer(text, **S.FIXTURES[name])
    n_all, _ = against_the_writer(text, keep_all=True, **S.FIXTURES[name])
    assert compared == n and n_all >= n and n_all > 0


def test_restatement_on_the_extended_realistic_input():
    text, n, _ = S.extended_realistic()
    for flags in (dict(min_identity=0.95), dict(min_identity=0.95, sensitive=True), dict(min_identity=0.95, min_overlap_percent=0.51),
                  dict(max_mismatch=3, min_length=300, max_length=400, keep_all=True), dict(min_identity=0.9, min_overlap=150)):
        written, compared = against_the_writer(text, **flags)
        assert written == compared and (written == n or "min_overlap" in flags or "min_overlap_percent" in flags)


def test_restatement_on_odd_inputs():
    """Interior spaces (full_seq is longer than the normalized record), lower case, U, short and empty records."""
    import random
    rng = random.Random(5)
    x, y, z = S.rand_seq(rng, 120), S.rand_seq(rng, 90), S.rand_seq(rng, 40)
    lower = (x + x[:60]).lower()
    rna = (y + y).replace(b"T", b"U")
    spaced = z[:20] + b" " + z[20:] + z[:10] + b" " + z[10:]
    text = (b">lower case\n" + lower + b"\n>rna\r\n" + rna[:70] + b"\r\n" + rna[70:] + b"\r\n>spaced id\n" + spaced +
            b"\n>short\nACGT\n>none\n" + S.rand_seq(rng, 200) + b"\n>empty\n\n>polyA\n" + b"A" * 77 + b"\n>spaces only\n" + b" " * 30 + b"\n")
    some = 0
    for flags in (dict(), dict(keep_all=True), dict(min_identity=0.9, sensitive=True), dict(max_mismatch=2, min_length=50),
                  dict(max_length=100, keep_all=True), dict(seed_length=5, min_overlap=30), dict(seed_length=5, min_overlap=22),
                  dict(seed_length=63, keep_all=True), dict(min_overlap_percent=0.4), dict(min_overlap_percent=0.55, keep_all=True),
                  dict(min_length=41), dict(min_length=40), dict(min_length=1000, keep_all=True)):
        some += against_the_writer(text, **flags)[0]
    assert some > 40


# ---- the worker's pre-check is subsumed --------------------------------------------------------------------------------
def subsumption_records(seed_len):
    data, offs = S.rolling(3, [300] * 40, pmin=40, pmax=120)
    seqs = [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(40)]
    data, offs = S.random_records(4, [300] * 10 + list(range(0, 2 * seed_len + 3)))
    seqs += [bytes(data[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)]
    import random
    rng = random.Random(6)
    seqs += [S.periodic(rng, n, max(1, n // 3)) for n in range(0, 3 * seed_len + 2)]
    seqs += [b"A" * n for n in (seed_len - 1, seed_len, seed_len + 1, 2 * seed_len - 1, 2 * seed_len, 2 * seed_len + 1, 300)]
    return seqs


@pytest.mark.parametrize("seed_len", (5, 10))
@pytest.mark.parametrize("sensitive", (False, True))
def test_the_workers_precheck_needs_no_step(seed_len, sensitive):
    """Every end the Monomerizer returns lies in [seed_len, n - seed_len], so a record shorter than the seed has none and one
    shorter than --min-length fails the writer's own min_length: the writer gives the same output with and without the
    pre-check applied to the ends."""
    seqs = subsumption_records(seed_len)
    data, offs = S.pack(seqs)
    found = 0
    for cut in (dict(max_mismatch=0), dict(max_mismatch=3), dict(min_identity=0.9)):
        ends = R.batch(data, offs, threads=2, seed_len=seed_len, sensitive=sensitive, **cut)
        for s, e in zip(seqs, ends):
            if int(e) != R.NONE:
                assert seed_len <= int(e) <= len(s) - seed_len, (len(s), int(e))
                found += 1
        recs = [(b"r%d" % i, s) for i, s in enumerate(seqs)]
        plain = [None if int(e) == R.NONE else int(e) for e in ends]
        for n in sorted({len(s) for s in seqs if len(s) in (0, seed_len, 2 * seed_len, 300)}):
            for min_length in sorted({0, seed_len, max(n - 1, 0), n, n + 1}):
                checked = [None if (len(s) < seed_len or len(s) < min_length) else e for s, e in zip(seqs, plain)]
                for keep_all in (False, True):
                    kw = dict(min_length=min_length, keep_all=keep_all, table_delim=b",")
                    assert R.write_records(recs, plain, **kw) == R.write_records(recs, checked, **kw), (n, min_length, keep_all)
                    # and the compact's restatement writes the same records with the same lengths
                    _, out_off, out_src, _ = MR.compact(data, offs, ends, min_length=min_length, keep_all=keep_all)
                    rows = R.write_records(recs, checked, **kw)[1].split(b"\n")[1:-1]
                    assert [r.split(b",")[0] for r in rows] == [recs[int(i)][0] for i in out_src]
                    assert [int(r.split(b",")[2]) for r in rows] == (out_off[1:] - out_off[:-1]).tolist()
    assert found > 100


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_filter_boundary_expectations_hold_in_the_restatement():
    for name, lengths, ends, full_len, flt, kept in MS.filter_boundary_cases():
        k, w, wl = MR.decide(lengths, ends, full_len, **flt)
        assert (int(k[0]) != MR.NONE) == kept == bool(w[0]), name
        assert int(wl[0]) == (ends[0] if kept else lengths[0]), name
        k2, w2, wl2 = MR.decide(lengths, ends, full_len, **dict(flt, keep_all=True))
        assert bool(w2[0]) and int(k2[0]) == int(k[0]) and int(wl2[0]) == int(wl[0])


# ---- the Python surface (no GPU needed: the library loads without one) ---------------------------------------------------
def test_filter_constructor_and_signatures():
    import __graft_entry__ as g
    g.build()
    from circkit_amd import api
    import circkit_amd
    f = api.monomer_filter()
    assert (f.min_length, f.max_length, f.min_overlap, f.use_min_overlap_percent, f.keep_all) == (0, 2 ** 64 - 1, 0, 0, 0)
    f = api.monomer_filter(min_length=5, max_length=70, min_overlap=9, min_overlap_percent=0.51, keep_all=True)
    assert (f.min_length, f.max_length, f.min_overlap, f.min_overlap_percent, f.use_min_overlap_percent, f.keep_all) == (5, 70, 9, 0.51, 1, 1)
    assert ctypes.sizeof(api.MonomerFilter) == 40          # 3 x uint64, a double, 2 x uint32: no padding
    for name in ("circkit_monomers_compact_device", "circkit_monomers_status", "circkit_monomers_batch"):
        assert name in api.SIGNATURES and hasattr(circkit_amd.load_library(), name)
    assert len(api.SIGNATURES["circkit_monomers_compact_device"][1]) == 11 and len(api.SIGNATURES["circkit_monomers_batch"][1]) == 12
    assert callable(circkit_amd.monomers_batch) and callable(circkit_amd.monomer_filter)
    for m in ("monomers_compact_device", "monomers_status", "monomers_batch"):
        assert callable(getattr(api.Context, m))
