"""CPU-only checks behind the uniq compact: the restatement the GPU is compared with (tests/uniq_compact_ref.py) against
oracle.cli_uniq on the reference's fixtures, the kernel's decision (ck_compact::decide_uniq, built for the host) against the
restatement's keep mask, and the ABI / Python surface of the three new entry points."""
import os

import numpy as np
import pytest

from tests import mono_sets as S
from tests import uniq_compact_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("circkit_uniq_compact_device", "circkit_uniq_compact_status", "circkit_uniq_batch")


# ---- the surface (no GPU needed: the library loads without one) ----------------------------------------------------------
def test_header_signatures_and_python_surface():
    import __graft_entry__ as g
    g.build()
    from tests.test_abi import header_symbols
    from circkit_amd import api
    import circkit_amd
    syms = header_symbols()
    for name in NEW:
        assert name in syms, "include/circkit.h does not declare %s" % name
        assert name in api.SIGNATURES and hasattr(circkit_amd.load_library(), name)
    assert len(api.SIGNATURES["circkit_uniq_compact_device"][1]) == 11 and len(api.SIGNATURES["circkit_uniq_batch"][1]) == 10
    assert len(api.SIGNATURES["circkit_uniq_compact_status"][1]) == 3
    for m in ("uniq_compact_device", "uniq_compact_status", "uniq_batch"):
        assert callable(getattr(api.Context, m))
    assert callable(circkit_amd.uniq_batch)


# ---- the restatement against the pinned writer ---------------------------------------------------------------------------
def records_of(text):
    """[(head, raw, normalized)] and the device's view of them: canonical bytes, offsets, first_seen."""
    from oracle import oracle as O
    recs = [(h, raw, O.normalize(raw)[0]) for h, raw in O.read_fasta(text)]
    data, offs = S.pack([r[2] for r in recs])
    canon, hashes = O.canonicalize_batch(data, offs, True, True, threads=2)
    return recs, data, canon, offs, O.uniq_first_seen(hashes)


def against_the_writer(text, canonical_out):
    from oracle import oracle as O
    fasta, table = O.cli_uniq(text, canonical_out=canonical_out)
    recs, data, canon, offs, fs = records_of(text)
    res = UR.compact(canon if canonical_out else data, offs, fs)
    UR.assert_equal(res, UR.compact_slow(canon if canonical_out else data, offs, fs), "vectorized against plain")
    out, out_off, out_src, dup_src, dup_first = res
    written = O.read_fasta(fasta)
    # the records written are the slices of out_src
    assert [h for h, _ in written] == [recs[int(i)][0] for i in out_src], "another set of records is written"
    for j, (head, seq) in enumerate(written):
        mine = bytes(out[int(out_off[j]):int(out_off[j + 1])])
        if canonical_out:
            assert seq == mine, head                           # :55 writes the canonical bytes as they are
        else:
            assert seq == recs[int(out_src[j])][1] and O.normalize(seq)[0] == mine, head     # :58 writes record.seq(); the batch holds it normalized
    # the table's rows are (id[dup_first[k]], id[dup_src[k]]) under the header "id,duplicate_id"
    ids = [O.record_id(r[0]) for r in recs]
    rows = b"".join(O.csv_row([ids[int(f)], ids[int(d)]], b",") for d, f in zip(dup_src, dup_first))
    assert table == ((b"id,duplicate_id\n" + rows) if len(dup_src) else b"")
    assert len(out_src) + len(dup_src) == len(recs)
    return len(out_src), len(dup_src)


@pytest.mark.parametrize("canonical_out", (False, True))
@pytest.mark.parametrize("name", ("repeated", "multiple_sequences", "simple"))
def test_restatement_on_the_cli_fixtures(name, canonical_out):
    text = open(os.path.join(S.EXAMPLES, name, "in.fasta"), "rb").read()
    kept, dropped = against_the_writer(text, canonical_out)
    assert kept >= 1 and (dropped >= 1 or name != "repeated")


def test_restatement_on_planted_duplicates():
    """Rotations and reverse complements of earlier records, an empty record twice, a record three times."""
    import random
    from oracle import oracle as O
    rng = random.Random(3)
    seqs = [S.rand_seq(rng, rng.randint(20, 90)) for _ in range(30)]
    seqs += [seqs[3][7:] + seqs[3][:7], O.revcomp(seqs[5]), b"", seqs[9], b"", seqs[9].lower(), O.revcomp(seqs[3])]
    rng.shuffle(seqs)
    text = b"".join(b">r%d some text\n%s\n" % (i, s) for i, s in enumerate(seqs))
    for canonical_out in (False, True):
        kept, dropped = against_the_writer(text, canonical_out)
        assert (kept, dropped) == (31, 6)


def test_restatement_other_bases_and_values():
    """base_index moves the kept value; an index of an earlier batch, ~0 and a LATER index all drop."""
    rng = np.random.default_rng(8)
    from tests import monomers_sets as MS
    data, offs = MS.batch(rng, [3, 0, 5, 1, 0, 2])
    base = 2 ** 40 + 7
    fs = np.array([base, 5, base + 2, UR.NOT_FOUND, base + 4, base + 6], dtype=np.uint64)
    out, out_off, out_src, dup_src, dup_first = UR.compact(data, offs, fs, base)
    assert out_src.tolist() == [0, 2, 4] and out_off.tolist() == [0, 3, 8, 8]
    assert dup_src.tolist() == [1, 3, 5] and dup_first.tolist() == [5, UR.NOT_FOUND, base + 6]
    assert bytes(out) == bytes(data[0:3]) + bytes(data[3:8])
    UR.assert_equal(UR.compact_slow(data, offs, fs, base), (out, out_off, out_src, dup_src, dup_first))
    assert not UR.keep_mask(fs, 0).any()


# ---- the kernel's decision, built for the host ---------------------------------------------------------------------------
def test_decide_uniq_on_random_triples():
    from tests.emu import uniq_compact_emu as E
    rng = np.random.default_rng(17)
    n = 5000
    for base in (0, 1, 2 ** 40 + 7, 2 ** 63, 2 ** 64 - n - 1):
        lengths = rng.integers(0, 2 ** 40, size=n, dtype=np.uint64)
        lengths[rng.random(n) < 0.2] = 0
        own = (np.uint64(base) + np.arange(n, dtype=np.uint64))
        kind = rng.integers(0, 6, size=n)
        fs = own.copy()
        earlier = own - rng.integers(1, 1000, size=n).astype(np.uint64)            # an earlier record (of an earlier batch, for small i)
        fs = np.where(kind == 1, earlier, fs)
        fs = np.where(kind == 2, np.uint64(UR.NOT_FOUND), fs)
        fs = np.where(kind == 3, own + np.uint64(1), fs)                            # nothing uniq produces; still a drop
        fs = np.where(kind == 4, own ^ np.uint64(1 << 32), fs)                      # equal in the low word only
        fs = fs.astype(np.uint64)
        kept, wlen = E.decide(lengths, fs, base)
        exp = UR.keep_mask(fs, base)
        assert np.array_equal(kept, exp), base
        assert np.array_equal(wlen, np.where(exp, lengths, np.uint64(0))), base
        assert 0 < exp.sum() < n
