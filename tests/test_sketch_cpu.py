"""CPU-only: the sketch surface of the ABI, the yardstick tests/sketch_ref.py against the known answers of the definition, and the
device routines of circkit_amd/csrc/sketch.h run as fibers by a stand-alone program (tests/emu/sketch_emu_main.cpp) against the
yardstick: every bin, every count, every (match, filled)."""
import numpy as np
import pytest

from tests import sketch_ref as R
from tests import sketch_sets as S

NAMES = {"circkit_sketch_batch_device": 7, "circkit_sketch_status": 3, "circkit_sketch_compare_device": 9, "circkit_sketch_compare_status": 2,
         "circkit_sketch_batch": 7, "circkit_sketch_compare": 9}
_C = S.constants()
SEG = _C["SKETCH_SEG"]


# ---- 1. the surface ----------------------------------------------------------------------------------------------------------
def test_the_surface():
    import ctypes
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
    for method in ("sketch_batch_device", "sketch_status", "sketch_compare_device", "sketch_compare_status", "sketch_batch", "sketch_compare"):
        assert callable(getattr(api.Context, method))
    for fn in ("sketch_params", "sketch_batch", "sketch_similarity"):
        assert callable(getattr(circkit_amd, fn))
    assert circkit_amd.SKETCH_EMPTY == R.EMPTY == 2 ** 64 - 1
    assert ctypes.sizeof(api.SketchParams) == 24
    p = circkit_amd.sketch_params()
    assert (p.k, p.log2_bins, p.seed, tuple(p.reserved)) == (21, 8, 0, (0, 0))
    p = circkit_amd.sketch_params(k=31, log2_bins=10, seed=2 ** 64 - 2)
    assert (p.k, p.log2_bins, p.seed) == (31, 10, 2 ** 64 - 2)
    header = open(os.path.join(ROOT, "include", "circkit.h")).read()
    assert "#define CIRCKIT_SKETCH_EMPTY 0xFFFFFFFFFFFFFFFFull" in header
    assert re.search(r"uint32_t k;.*?uint32_t log2_bins;.*?uint64_t seed;.*?uint32_t reserved\[2\];.*?\} circkit_sketch_params;", header, flags=re.S)


# ---- 2. the yardstick --------------------------------------------------------------------------------------------------------
KNOWN_ROW = {1: 0x1ef1a10b70ffd85b, 7: 0x7ed3adb081e15aec, 9: 0x9d178c809a5ff049, 10: 0xaadedba47699223e, 11: 0xb93e2d401bd06ce8,
             13: 0xd385d44613e0daf3, 14: 0xe8b4b3b1c77c4573}


def known_records():
    rng = np.random.default_rng(822)
    return (b"ACGTACGTTGCA", S.with_symbol(S.random_acgt(rng, 822), [400]))


def test_known_answers():
    assert R.fmix64(0) == 0 and R.fmix64(1) == 0xb456bcfc34c2cb2c
    row, n = R.sketch(b"ACGTACGTTGCA", 4, 4, 0)
    assert n == 12 and {b: v for b, v in enumerate(row) if v != R.EMPTY} == KNOWN_ROW
    assert R.sketch(known_records()[1], 21, 8)[1] == 822 - 21 == 801


def test_the_yardstick_spelled_out_symbol_by_symbol():
    """The k-mers once more without int(): digit by digit, with the reverse complement built from the k-mer itself."""
    rng = np.random.default_rng(3)
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    for k, n in ((4, 4), (5, 23), (21, 60), (32, 40), (16, 15)):
        seq = S.with_symbol(S.random_acgt(rng, n), [n // 2], b"N" if k == 5 else b"A")
        want = []
        for p in range(n if n >= k else 0):
            kmer = [seq[(p + i) % n] for i in range(k)]
            if any(b not in code for b in kmer):
                continue
            f = r = 0
            for b in kmer:
                f = f * 4 + code[b]
            for b in reversed(kmer):
                r = r * 4 + (3 - code[b])
            want.append(R.fmix64(min(f, r) ^ 77))
        assert R.kmer_hashes(seq, k, 77) == want and (len(want) > 0) == (n >= k)


def test_fmix64_inverse():
    rng = np.random.default_rng(4)
    for v in [0, 1, R.EMPTY, 2 ** 63] + [int(x) for x in rng.integers(0, 2 ** 64, size=200, dtype=np.uint64)]:
        assert R.fmix64(R.fmix64_inverse(v)) == v and R.fmix64_inverse(R.fmix64(v)) == v


def test_the_row_is_invariant_in_the_yardstick():
    rng = np.random.default_rng(5)
    for n in (21, 22, 100, 333):
        s = S.with_symbol(S.random_acgt(rng, n), [n // 3])
        base = R.sketch(s, 21, 6, 9)
        for r in (1, 7, n - 1):
            assert R.sketch(s[r:] + s[:r], 21, 6, 9) == base
        assert R.sketch(R.revcomp(s), 21, 6, 9) == base
        assert R.sketch(s + s, 21, 6, 9)[0] == base[0] and R.sketch(s + s, 21, 6, 9)[1] == 2 * base[1]


def test_compare_pairs_is_compare():
    rng = np.random.default_rng(6)
    rows = S.compare_rows(rng, 4)
    pairs = [(i, j) for i in range(10) for j in range(10)] + [(len(rows), 0), (0, len(rows)), (2 ** 32 - 1, 2 ** 32 - 1)]
    match, filled, bad = R.compare_pairs(rows, rows, pairs)
    assert bad == 3 and (match[-3:] == 0).all() and (filled[-3:] == 0).all()
    for (i, j), m, f in zip(pairs[:-3], match, filled):
        assert R.compare(rows[i], rows[j]) == (m, f)
    assert R.compare(rows[0], rows[1]) == (16, 16) and R.compare(rows[0], rows[2]) == (0, 16) and R.compare(rows[3], rows[4]) == (0, 0)
    assert R.compare(rows[0], rows[3]) == (0, 16) and R.compare(rows[0], rows[5]) == (8, 16)


def test_usefulness_of_the_inputs():
    """The yardstick alone: planted pairs (1 % substitutions, a rotation, a strand) score at least 0.3, unrelated pairs at most 0.05."""
    records, planted, unrelated = S.planted(S.USEFUL_SEED)
    rows, _ = S.expected(records, 21, 8)
    m, f, _ = R.compare_pairs(rows, rows, planted)
    assert (m / f).min() >= 0.3
    m, f, _ = R.compare_pairs(rows, rows, unrelated)
    assert (m / f).max() <= 0.05



# ---- 3. the device routines on the CPU ---------------------------------------------------------------------------------------
def test_constants():
    from tests.emu import sketch_emu
    assert sketch_emu.constants() == (SEG, _C["SKETCH_WAVES"])
    assert {SEG - 1, SEG, SEG + 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + 21 - 2} <= set(S.lengths(21))
    assert set(S.lengths(21, 512)) != set(S.lengths(21))


def test_fmix64_as_compiled(tmp_path):
    from tests.emu import sketch_emu
    words = np.random.default_rng(8).integers(0, 2 ** 64, size=1000, dtype=np.uint64)
    words[:3] = [0, 1, 2 ** 64 - 1]
    got = sketch_emu.fmix64(words, tmp_path)
    assert [int(v) for v in got] == [R.fmix64(int(v)) for v in words]


def check(got, records, k, log2_bins, seed, what):
    rows, counts, valid, unprocessed, n_long = got
    exp_rows, exp_counts = S.expected(tuple(records), k, log2_bins, seed)
    assert np.array_equal(counts, exp_counts), what
    assert np.array_equal(rows, exp_rows), what
    assert valid == int(exp_counts.sum()) and unprocessed == 0 and n_long == sum(len(s) > SEG for s in records), what


def test_known_answers_as_fibers(tmp_path):
    from tests.emu import sketch_emu
    a, b = known_records()
    got = sketch_emu.run_sketch([(*S.pack([a]), dict(k=4, log2_bins=4), {}), (*S.pack([b]), dict(k=21, log2_bins=8), {})], tmp_path)
    assert {i: int(v) for i, v in enumerate(got[0][0][0]) if v != R.EMPTY} == KNOWN_ROW and got[0][1][0] == 12
    assert got[1][1][0] == 801 and got[1][2] == 801


def test_every_length_as_fibers(tmp_path):
    """Every length of the set under every (k, bins) of the list, the payload start moving through the 16 alignments, offsets[0]
    not 0, workgroup counts on both sides of the number of long records."""
    from tests.emu import sketch_emu
    cases = []
    for i, (k, b) in enumerate(S.PARAMS):
        recs = S.length_records(k)
        cases.append((*S.pack(recs), dict(k=k, log2_bins=b, seed=i % 2 * 0x9E3779B97F4A7C15), dict(lead=3 * i + 1, in_shift=(5 * i) % 16, long_grid=(1, 4, 16)[i % 3])))
    got = sketch_emu.run_sketch(cases, tmp_path)
    for (k, b), case, g in zip(S.PARAMS, cases, got):
        check(g, S.length_records(k), k, b, case[2]["seed"], (k, b))


def test_symbols_and_alignments_as_fibers(tmp_path):
    from tests.emu import sketch_emu
    cases, names = [], []
    for shift in range(16):
        k, b, seed = ((21, 8, 0), (4, 4, 5), (32, 6, 2 ** 64 - 1), (16, 10, 1))[shift % 4]
        recs = tuple(s for _, s in S.symbol_records(k))
        cases.append((*S.pack(recs), dict(k=k, log2_bins=b, seed=seed), dict(lead=shift % 3, in_shift=shift, short_grid=1 + shift % 5, counts=shift != 7)))
        names.append((recs, k, b, seed))
    got = sketch_emu.run_sketch(cases, tmp_path)
    for shift, ((recs, k, b, seed), g) in enumerate(zip(names, got)):
        if g[1] is None:
            g = (g[0], S.expected(recs, k, b, seed)[1], *g[2:])
        check(g, recs, k, b, seed, shift)
    # what the set is for: every position of the N kills k k-mers, the wrap included; nothing survives all N or lower case
    exp = dict(zip([n for n, _ in S.symbol_records(21)], S.expected(tuple(s for _, s in S.symbol_records(21)), 21, 8)[1]))
    assert all(exp["N at %d" % p] == 40 - 21 for p in range(40)) and exp["all N"] == exp["lower case"] == 0 and exp["one lower"] == 70 - 21
    assert exp["poly-A"] == 100 and exp["N on both sides"] == 2 * SEG + 500 - 2 * 22


def test_the_hash_that_equals_empty_as_fibers(tmp_path):
    from tests.emu import sketch_emu
    seed = S.poly_a_seed_for_empty(21)
    assert R.fmix64(0 ^ seed) == R.EMPTY
    recs = (b"A" * 100, b"T" * 30, b"A" * (SEG + 9), b"ACGT" * 20)
    got = sketch_emu.run_sketch([(*S.pack(recs), dict(k=21, log2_bins=8, seed=seed), {})], tmp_path)[0]
    check(got, recs, 21, 8, seed, "h = EMPTY")
    assert (got[0][:3] == np.uint64(R.EMPTY)).all() and got[1].tolist()[:3] == [100, 30, SEG + 9] and (got[0][3] != np.uint64(R.EMPTY)).any()


def test_a_record_of_2_to_the_31_is_not_read_as_fibers(tmp_path):
    """Crafted offsets over a payload of 10 bytes in an exactly sized block: the record of 2^31 symbols and the one whose offsets
    decrease get EMPTY rows and count 0 and are counted; reading either would leave the block."""
    from tests.emu import sketch_emu
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    for offs in ([0, 10, 10 + 2 ** 31], [0, 10, 4], [0, 10, 10 + 2 ** 40]):
        rows, counts, valid, unprocessed, n_long = sketch_emu.run_sketch([(data, np.array(offs, dtype=np.uint64), dict(k=4, log2_bins=4), dict(lead=2))], tmp_path)[0]
        exp = S.expected((b"ACGTACGTAC",), 4, 4)
        assert np.array_equal(rows[0], exp[0][0]) and (rows[1] == np.uint64(R.EMPTY)).all()
        assert counts.tolist() == [10, 0] and (valid, unprocessed, n_long) == (10, 1, 0)


def test_compare_as_fibers(tmp_path):
    from tests.emu import sketch_emu
    rng = np.random.default_rng(10)
    cases = []
    for b in S.LOG2_BINS:
        a, other = S.compare_rows(rng, b), S.compare_rows(rng, b, n=9)
        other[2] = a[0]
        na, nb = len(a), len(other)
        same_pairs = [(i, j) for i in range(10) for j in range(10)] + [(3, na), (na, 3), (5, 5), (2 ** 32 - 1, 0), (0, 2 ** 32 - 1), (1, 0)]
        diff_pairs = [(i, j) for i in range(na) for j in range(nb)] + [(na, 0), (0, 0), (0, nb), (nb, 2), (2 ** 32 - 1, 2 ** 32 - 1), (0, 2)]
        cases += [(a, None, same_pairs, 3), (a, other, diff_pairs, 64), (a, other, [], 2)]
    got = sketch_emu.run_compare(cases, tmp_path)
    for (a, other, pairs, _), (match, filled, bad) in zip(cases, got):
        m, f, n_bad = R.compare_pairs(a, a if other is None else other, pairs)
        assert bad == n_bad and np.array_equal(match, m) and np.array_equal(filled, f)
        assert not pairs or (bad >= 3 and match.max() == a.shape[1])


def test_a_payload_across_byte_2_32_as_fibers(tmp_path):
    """Every length of the set, and one record of three spans and a tail in their middle, with the payload 2^32 bytes, less half
    that record, into a lazily reserved buffer (tests/high_base.py, "middle"): byte 2^32 of the buffer lies inside the record's second
    span, half of the short records lie wholly above it, and payload positions need 33 bits."""
    from tests import high_base as H
    from tests.emu import sketch_emu
    recs, j, seg = H.sketch_records("lengths", 21)
    data, offs = S.pack(recs)
    lead = int(H.conditions(data, offs, j, "middle")[0])
    got = sketch_emu.run_sketch([(data, offs, dict(k=21, log2_bins=8, seed=3), dict(lead=lead, in_shift=7, long_grid=4))], tmp_path)[0]
    check(got, recs, 21, 8, 3, "across 2^32")
    assert got[4] >= 4                                                          # (the records of more than one span)
