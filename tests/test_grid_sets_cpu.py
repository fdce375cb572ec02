"""CPU-only: the inputs of tests/test_grid_stride_gpu.py do what their names say.  From the launch constants read out of the
sources, the busiest workgroup of every fixed-grid kernel makes a second trip (a third for the FASTA parser) on its input, and
the long sketch kernel's inputs reach the work-sharing shapes they claim: a GPU test that merely passes proves nothing if its
input is too small.  The helpers the large sets are checked with (periodic_protein, replicated) are held against the plain
yardsticks, and the small-grid versions of the long_block shapes run as fibers against tests/sketch_ref.py."""
import numpy as np
import pytest

from tests import grid_sets as G
from tests import sketch_ref
from tests import sketch_sets

C = G.grid_constants()
SEG = C["SKETCH_SEG"]


# ---- the constants -----------------------------------------------------------------------------------------------------------
def test_constants_agree_with_the_units_own_readers():
    from tests import monomers_sets, translate_sets, windows_sets
    assert C["COMPACT_TILE_BYTES"] == monomers_sets.constants()["TILE_BYTES"]
    assert C["WINDOWS_TILE_BYTES"] == windows_sets.constants()["TILE_BYTES"]
    assert C["TILE_RESIDUES"] == translate_sets.constants()["TILE_RESIDUES"]
    assert (C["SKETCH_SEG"], C["SKETCH_WAVES"]) == tuple(sketch_sets.constants()[k] for k in ("SKETCH_SEG", "SKETCH_WAVES"))
    assert all(isinstance(v, int) and v > 0 for v in C.values())


def test_constants_agree_with_the_fiber_programs():
    from tests.emu import fasta_emu, fasta_write_emu, sketch_emu
    assert C["FASTA_TILE_BYTES"] == fasta_emu.constants()["TILE_BYTES"]
    assert C["WRITE_TILE_BYTES"] == fasta_write_emu.constants()["TILE_BYTES"]
    assert sketch_emu.constants() == (C["SKETCH_SEG"], C["SKETCH_WAVES"])


def test_trips_and_long_trips():
    assert [G.trips(n, 4) for n in (0, 1, 4, 5, 8, 9)] == [0, 1, 1, 2, 2, 3]
    assert G.long_trips([], 5) == (0, 0, 5)
    # fewer records than workgroups, none over: 2 records on 8 workgroups of 4 waves share 16 spans a record and round
    assert G.long_trips([17 * SEG, SEG + 1], 8) == (2, 1, 0)
    assert G.long_trips([SEG + 1] * 3, 5) == (1, 1, 2)
    assert G.long_trips([SEG + 1] * 7, 5) == (2, 2, 0)
    assert G.long_trips([9 * SEG], 2) == (2, 1, 0)
    assert G.long_trips([9 * SEG + 5] * 5, 5) == (3, 1, 0)


# ---- every GPU case reaches its path -----------------------------------------------------------------------------------------
def test_the_fasta_text_makes_three_trips_and_holds_what_it_names():
    text, m = G.fasta_text()
    grid, T = C["FASTA_GRID"], C["FASTA_TILE_BYTES"]
    tiles = -(-len(text) // T)
    assert tiles == 2 * grid + 3 and G.trips(tiles, grid) == 3
    # a record start on the last byte of tile grid - 1; its header covers tile grid whole and ends in tile grid + 1
    at = m["start_last"]
    assert at == grid * T - 1 and text[at - 1:at + 1] == b"\n>"
    end = text.index(b"\n", at)
    assert (grid + 1) * T < end < (grid + 2) * T
    # a record start on the first byte of a second-trip tile
    at = m["start_first"]
    assert at % T == 0 and grid < at // T < 2 * grid and text[at - 1:at + 1] == b"\n>"
    # a second-trip tile of dropped bytes only
    assert m["blank"] <= (grid + 5) * T and m["blank_end"] >= (grid + 6) * T and set(text[m["blank"]:m["blank_end"]]) == set(b"\n \t\r")
    # one line of one base from a second-trip tile through a third-trip one
    assert m["poly"] // T == 2 * grid - 1 and m["poly_end"] // T == 2 * grid + 1
    assert set(text[m["poly"]:m["poly_end"]]) == {ord("A")} and text[m["poly"] - 1] == text[m["poly_end"]] == ord("\n")
    assert text[m["crlf"]:m["crlf_end"]].count(b"\r\n") > 300 and b"\r\n" not in text[m["crlf_end"]:]
    assert text.startswith(b">") and not text.endswith(b"\n")


def test_the_compact_batch_keeps_a_second_trip():
    data, offs, keep = G.compact_batch()
    grid, T = C["COMPACT_GATHER_GRID"], C["COMPACT_TILE_BYTES"]
    lengths = np.diff(offs.astype(np.int64))
    kept = int(lengths[keep].sum())
    assert (grid + 5) * T + 77 <= kept < (grid + 5) * T + 77 + 1000
    assert G.trips(-(-kept // T), grid) == 2
    big = int(np.argmax(lengths))
    assert len(lengths) == 36_001 and big == 18_000 and lengths[big] == 3_000_000 and keep[big] and len(data) == offs[-1]
    assert len({data[int(a):int(a) + 1000].tobytes() for a in offs[:18_000]}) <= 600
    ends, fs = G.compact_ends(offs, keep), G.compact_first_seen(keep)
    assert np.array_equal(ends != 0xFFFFFFFF, keep) and np.array_equal(fs == np.arange(len(keep), dtype=np.uint64), keep)
    dropped = fs[~keep]
    assert (dropped == np.uint64(2 ** 64 - 1)).any() and (dropped < np.flatnonzero(~keep).astype(np.uint64)).any()


@pytest.mark.parametrize("which", ["gather", "translate"])
def test_the_window_sets_write_a_second_trip(which):
    from tests import windows_ref
    data, offs, wins, segments = G.gather_set() if which == "gather" else G.translate_set()
    unit, T = (1, C["WINDOWS_TILE_BYTES"]) if which == "gather" else (3, C["TILE_RESIDUES"])
    grid = C["WINDOWS_GATHER_GRID"]
    lengths = np.diff(offs.astype(np.int64))
    assert len(lengths) == 16 and {1, 2, 5000} <= set(lengths.tolist())
    invalid = np.array([windows_ref.is_invalid(w, lengths) for w in wins])
    units = np.where(invalid | (lengths[np.minimum(wins["record"], 15)] == 0), 0, wins["length"] // np.uint64(unit)).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(units)])
    total = int(cum[-1])
    assert (grid + 3) * T < total <= (grid + 3) * T + 200 and G.trips(-(-total // T), grid) == 2
    long = [lo for kind, lo, hi in segments if kind == "long"]
    small = np.ones(len(wins), dtype=bool)
    small[long] = False
    assert len(long) == G.N_LONG_WINDOWS and int((small & ~invalid).sum()) == G.N_SMALL_WINDOWS + 1 and 4 <= int(invalid.sum()) <= 10
    assert (units[long] > 500_000).all() and (units[small] < T).all() and units[small & ~invalid].min() >= 1
    assert set(lengths[wins["record"][long]].tolist()) == set(lengths[lengths > 0].tolist()) and set(wins["strand"][long].tolist()) == {0, 1}
    assert (wins["start"][long] >= lengths[wins["record"][long]]).any() and (wins["start"][long] < lengths[wins["record"][long]]).any()
    # small windows at the front, round output unit grid * tile, and at the end
    at = int(np.searchsorted(cum, grid * T, side="right")) - 1
    assert small[0] and small[-1] and small[at - 300:at + 300].all() and 0 < units[at] <= 40
    assert cum[long[-1] + 1] < grid * T


def test_the_write_cases_write_a_second_trip():
    from tests import fasta_write_sets as W
    grid, T = C["WRITE_GRID"], C["WRITE_TILE_BYTES"]
    body, raw = G.write_cases()
    for c in (body, raw):
        recs, bad = W.expected(c)
        total = sum(len(r) for r in recs)
        assert bad == 0 and c.n_out == G.N_WRITE == len(recs) and G.trips(-(-total // T), grid) == 2
        assert len(set(c.src.tolist())) > 400 and c.n_src == G.N_WRITE
        if c is body:
            assert (grid + 2) * T < total <= (grid + 2) * T + G.N_WRITE
            assert recs[2].split(b"\n")[0].count(b"_RC_ORF") == 1 and b"_ORF" in recs[0].split(b"\n")[0] and b"_RC_ORF" not in recs[0]
        else:
            assert c.labels is None and all(r.count(b"\n") >= 15 for r in recs[:50])      # wrapped lines: the raw spans keep their line ends


@pytest.mark.parametrize("name", G.LONG_CASES)
def test_the_long_cases_reach_their_shapes(name):
    """Whatever order the device's list takes: the claims hold for the batch order, its reverse and a shuffle."""
    grid = C["LONG_GRID"]
    lengths = G.long_lengths(name)
    want_spans, want_entries, want_idle = G.LONG_CLAIMS[name]
    n_long = {"leftover_3": 3, "leftover_5": 5, "leftover_700": 700, "two_entries": grid + 5, "grid_exact": grid, "parts_one": 1100}[name]
    assert len(lengths) == n_long and len(G.long_case(name)) - n_long == {"two_entries": 1000, "grid_exact": 0, "parts_one": 30}.get(name, 50)
    for order in (lengths, lengths[::-1], list(np.random.default_rng(1).permutation(lengths))):
        spans, entries, idle = G.long_trips(order, grid)
        assert (spans >= 2) == want_spans and (entries >= 2) == want_entries and (idle > 0) == want_idle, (name, spans, entries, idle)
        if name.startswith("leftover"):
            assert idle == grid % n_long
        if name == "parts_one":
            assert idle == grid - n_long and grid // n_long == 1
        if name == "grid_exact":
            assert spans == 3 and lengths.count(9 * SEG + 5) == 4
    pool = G.long_pool()
    assert sum(len(s) > SEG for s in pool) == G.N_LONG_POOL and sum(len(s) for s in pool) <= 400_000


def test_the_short_set_makes_a_second_trip():
    distinct, order = G.short_set()
    waves = C["SKETCH_WAVES"]
    blocks = -(-len(order) // waves)
    grid = min(blocks, C["SHORT_MAX_GRID"])
    assert len(order) == 40_000 and len(distinct) == 300 and blocks > C["SHORT_MAX_GRID"] and G.trips(blocks, grid) == 2
    lens = np.array([len(s) for s in distinct])[order]
    assert {0, G.SHORT_K - 1, G.SHORT_K, 30, 333, SEG - 1, SEG, SEG + 1} == set(lens.tolist()) and int((lens == SEG + 1).sum()) == 40
    # a wave meets an empty, a short and a long record on its two trips, in either order
    first, second = lens[:len(lens) - grid * waves], lens[grid * waves:]
    kind = lambda n: np.where(n == 0, 0, np.where(n > SEG, 2, 1))
    met = set(zip(kind(first).tolist(), kind(second).tolist()))
    assert {(0, 1), (1, 0), (1, 2), (2, 1), (1, 1)} <= met


@pytest.mark.parametrize("log2_bins", [4, 8])
def test_the_compare_set_makes_a_second_trip(log2_bins):
    a, b, pairs = G.compare_set(log2_bins)
    blocks = -(-len(pairs) // C["COMPARE_WAVES"])
    grid = min(blocks, C["COMPARE_MAX_GRID"])
    assert len(pairs) == C["COMPARE_MAX_GRID"] * C["COMPARE_WAVES"] + 1000 and G.trips(blocks, grid) == 2
    assert a.shape == (G.N_COMPARE_A, 1 << log2_bins) and b.shape == (G.N_COMPARE_B, 1 << log2_bins)
    top = (a >> np.uint64(63)).astype(bool) & (a != np.uint64(sketch_ref.EMPTY))
    assert 0.2 < top.mean() < 0.8 and (a < np.uint64(2 ** 63)).any() and (a == np.uint64(sketch_ref.EMPTY)).any()
    m, f, bad = sketch_ref.compare_pairs(a, b, pairs[:5000])
    assert (m > 0).mean() > 0.5 and 0 < bad
    n_bad = int(((pairs[:, 0] >= len(a)) | (pairs[:, 1] >= len(b))).sum())
    assert 0.0005 < n_bad / len(pairs) < 0.002 and (pairs[-1, 1] >= len(b))


# ---- the helpers of the large sets against the plain yardsticks --------------------------------------------------------------
def test_periodic_protein_is_the_plain_translation():
    """Every record length 1..40, both strands, starts 0, n - 1 and n + 7, windows of 3n - 1, 3n, 3n + 1 and 7n + 2 symbols."""
    from tests import translate_ref, translate_sets, windows_ref
    rng = np.random.default_rng(41)
    alphabet = np.frombuffer(translate_sets.ALPHABET, dtype=np.uint8)
    tables = (translate_sets.DISTINCT, translate_ref.genetic_codes()[11])
    checked = 0
    for n in range(1, 41):
        data = alphabet[rng.integers(0, len(alphabet), size=n)]
        offs = np.array([0, n], dtype=np.uint64)
        rows = [(length, 0, start, strand) for strand in (0, 1) for start in (0, n - 1, n + 7) for length in (3 * n - 1, 3 * n, 3 * n + 1, 7 * n + 2)]
        aa, unknown = tables[n % 2], (b"!", b"X")[n % 2]
        exp, exp_off, bad = translate_ref.windows_translate(data, offs, windows_ref.windows(rows), aa, unknown)
        assert bad == 0
        exp = exp.tobytes()
        for k, (length, _, start, strand) in enumerate(rows):
            got = G.periodic_protein(data.tobytes(), start, strand, length // 3, aa, unknown)
            assert got == exp[int(exp_off[k]):int(exp_off[k + 1])], (n, length, start, strand)
            checked += 1
    assert checked == 40 * 24
    assert G.periodic_protein(b"", 0, 0, 5, tables[0]) == b"" and G.periodic_protein(b"ACG", 0, 0, 0, tables[0]) == b""


def test_translate_expected_is_the_plain_translation_on_a_small_list():
    """The segment-wise assembly of the large translate's answer, on a list small enough for the plain yardstick as a whole."""
    from tests import translate_ref, translate_sets, windows_ref
    data, offs, wins, segments = G.translate_set()
    keep = np.concatenate([np.arange(0, 40), np.arange(16_990, 17_002)])           # small windows and the two invalid ones
    long = windows_ref.windows([(3 * 700 + 1, 1, 0, 1), (3 * 701 + 2, 2, 1, 0), (3 * 9000, 15, 4999, 1)])
    small = wins[keep]
    w = np.concatenate([small[:40], long[:1], small[40:], long[1:]])
    seg = [("small", 0, 40), ("long", 40, 41), ("small", 41, 53), ("long", 53, 54), ("long", 54, 55)]
    aa = translate_ref.genetic_codes()[1]
    got = G.translate_expected(data, offs, w, seg, aa)
    exp = translate_ref.windows_translate(data, offs, w, aa)
    assert got[2] == exp[2] == 2 and np.array_equal(got[1], exp[1]) and np.array_equal(got[0], exp[0])


def sketch_sets_of_the_gpu_test():
    for name in G.LONG_CASES:
        yield name, G.long_pool(), G.long_case(name), G.LONG_K, G.LONG_LOG2_BINS
    yield ("short",) + G.short_set() + (G.SHORT_K, G.SHORT_LOG2_BINS)


@pytest.mark.parametrize("which", range(len(G.LONG_CASES) + 1), ids=list(G.LONG_CASES) + ["short"])
def test_replicated_is_the_direct_yardstick(which):
    """A 200-record sample of each sketch set, sketched directly, against the per-distinct answer indexed by the order."""
    name, distinct, order, k, log2_bins = list(sketch_sets_of_the_gpu_test())[which]
    rows, counts = sketch_sets.expected(tuple(distinct), k, log2_bins)
    exp_rows, exp_counts = G.replicated(rows, order), G.replicated(counts, order)
    assert exp_rows.shape == (len(order), 1 << log2_bins) and exp_counts.shape == (len(order),)
    sample = np.sort(np.random.default_rng(200 + which).choice(len(order), size=min(200, len(order)), replace=False))
    direct_rows, direct_counts = sketch_ref.sketch_batch([distinct[i] for i in order[sample]], k, log2_bins)
    assert np.array_equal(direct_rows, exp_rows[sample]) and np.array_equal(direct_counts, exp_counts[sample])
    assert G.replicated([b"ab", b"", b"c"], [2, 0, 0, 1]) == b"cabab"


# ---- the long_block shapes at small grids, as fibers -------------------------------------------------------------------------
def test_the_long_block_shapes_as_fibers(tmp_path):
    """n_long = 3 at grid 5 leaves workgroups over, n_long = 7 at grid 5 gives workgroups two list entries, one record of 9 spans
    at grid 2 gives each wave two spans: against tests/sketch_ref.py exactly.  Of these shapes tests/test_sketch_cpu.py holds one,
    two list entries per workgroup (test_every_length_as_fibers runs four long records on a grid of 1); it stays as it is."""
    from tests.emu import sketch_emu
    pool = G.long_pool()
    rng = np.random.default_rng(9)
    nine = sketch_sets.with_symbol(sketch_sets.random_acgt(rng, 8 * SEG + 77), [4 * SEG - 1, 4 * SEG, 8 * SEG - 1, 8 * SEG])
    sets = [("3 on 5", [pool[14], pool[0], pool[15], pool[6], pool[8], pool[13]], 5, (True, False, True)),
            ("7 on 5", [pool[i] for i in (0, 12, 1, 2, 16, 3, 4, 10, 5, 17)], 5, (True, True, False)),
            ("9 spans on 2", [pool[13], nine, pool[21]], 2, (True, False, False))]
    cases = []
    for k, (name, recs, grid, claims) in enumerate(sets):
        spans, entries, idle = G.long_trips([len(s) for s in recs if len(s) > SEG], grid)
        assert ((spans >= 2), (entries >= 2), (idle > 0)) == claims, (name, spans, entries, idle)
        cases.append((*sketch_sets.pack(recs), dict(k=G.LONG_K, log2_bins=G.LONG_LOG2_BINS, seed=k), dict(long_grid=grid, short_grid=2, lead=k, in_shift=3 * k)))
    got = sketch_emu.run_sketch(cases, tmp_path)
    for k, ((name, recs, grid, _), (rows, counts, valid, unprocessed, n_long)) in enumerate(zip(sets, got)):
        exp_rows, exp_counts = sketch_sets.expected(tuple(recs), G.LONG_K, G.LONG_LOG2_BINS, k)
        assert np.array_equal(counts, exp_counts) and np.array_equal(rows, exp_rows), name
        assert (valid, unprocessed, n_long) == (int(exp_counts.sum()), 0, sum(len(s) > SEG for s in recs)), name
