"""GPU: every kernel that launches a fixed number of workgroups and walks its work in a `for (t = blockIdx.x; t < n; t += gridDim.x)`
loop, on an input large enough for a second trip (a third for the FASTA parser), and the long sketch kernel in each of its
work-sharing shapes.  On that trip a workgroup reuses its LDS image, its wave counters and its carried state, and only the real
card preempts between the collectives of two trips.  The inputs are tests/grid_sets.py's; tests/test_grid_sets_cpu.py computes
from the sources' launch constants that each reaches its path.  Every comparison is exact, against the plain yardstick of the
unit, and the canaries of the unit's own GPU test surround every output."""
import numpy as np
import pytest

from tests import grid_sets as G

pytestmark = pytest.mark.gpu

C = G.grid_constants()
OK, INVALID_ARG = 0, -1


@pytest.fixture(scope="module")
def ctx():
    """A ctx that launches on torch's current stream, so that the tensors torch fills and the ctx's kernels are ordered."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


# ---- FASTA parse: fasta_bounds_kernel, fasta_summaries_kernel, fasta_apply_kernel ----------------------------------------------
@pytest.mark.parametrize("pair", range(4), ids=["first_final", "first", "final", "middle"])
def test_fasta_parse_three_trips(ctx, pair):
    """2 * FASTA_GRID + 3 tiles of text against the host packer: counts, offsets, payload, head and raw spans."""
    from tests import fasta_sets
    from tests import test_fasta_device_gpu as unit
    text, _ = G.fasta_text()
    first, final = fasta_sets.FLAG_PAIRS[pair]
    assert fasta_sets.deterministic(text, first, final)
    for in_shift in (0, 5):
        for out_shift in (0, 11):
            res = unit.parse(ctx, text, first, final, what=(pair, in_shift, out_shift), in_shift=in_shift, out_shift=out_shift)
            assert res["records"] > 16_000 and res["head"] is not None and res["raw"] is not None


def test_fasta_parse_three_trips_host_form(ctx):
    from circkit_amd import api
    text, _ = G.fasta_text()
    exp = api.fasta_parse(text)
    got = ctx.fasta_parse_text(text)
    assert got[0] == exp[0] and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]) and got[3] == exp[3]
    assert len(exp[0]) > 16_000


# ---- compact_gather_kernel: the monomer compact and the uniq compact -----------------------------------------------------------
def test_monomer_compact_past_the_grid(ctx):
    from tests import monomers_ref
    from tests import test_monomers_compact_gpu as unit
    data, offs, keep = G.compact_batch()
    ends = G.compact_ends(offs, keep)
    exp = monomers_ref.compact(data, offs, ends)
    assert len(exp[0]) >= (C["COMPACT_GATHER_GRID"] + 5) * C["COMPACT_TILE_BYTES"] + 77
    for out_shift in (0, 9):
        got = unit.run_device(ctx, data, offs, ends, out_shift=out_shift)
        monomers_ref.assert_equal(got, exp, out_shift)


def test_uniq_compact_past_the_grid(ctx):
    from tests import test_uniq_compact_gpu as unit
    from tests import uniq_compact_ref
    data, offs, keep = G.compact_batch()
    fs = G.compact_first_seen(keep)
    exp = uniq_compact_ref.compact(data, offs, fs)
    assert len(exp[0]) >= (C["COMPACT_GATHER_GRID"] + 5) * C["COMPACT_TILE_BYTES"] + 77 and len(exp[3]) == len(exp[4]) == int((~keep).sum())
    for out_shift in (0, 9):
        unit.check(ctx, data, offs, fs, what="past the grid", exp=exp, out_shift=out_shift)       # d_dup_src / d_dup_first included


# ---- windows_gather_kernel, windows_translate_kernel -------------------------------------------------------------------------
def test_windows_gather_past_the_grid(ctx):
    from tests import test_windows_gpu as unit
    from tests import windows_ref
    data, offs, wins, _ = G.gather_set()
    exp = windows_ref.gather(data, offs, wins)
    assert len(exp[0]) > (C["WINDOWS_GATHER_GRID"] + 3) * C["WINDOWS_TILE_BYTES"] and exp[2] > 0
    for out_shift in (0, 13):
        unit.check(ctx, data, offs, wins, what=out_shift, exp=exp, out_shift=out_shift)


@pytest.mark.parametrize("table", [11, 1])
def test_windows_translate_past_the_grid(ctx, table):
    """The long windows against periodic_protein, the small and invalid ones against translate_ref.windows_translate."""
    from tests import test_translate_gpu as unit
    from tests import translate_ref
    data, offs, wins, segments = G.translate_set()
    code = (translate_ref.genetic_codes()[table], b"X", False)
    exp = G.translate_expected(data, offs, wins, segments, code[0], code[1])
    assert len(exp[0]) > (C["WINDOWS_GATHER_GRID"] + 3) * C["TILE_RESIDUES"] and exp[2] > 0
    for out_shift in (0, 13):
        unit.check(ctx, data, offs, wins, code, what=(table, out_shift), exp=exp, out_shift=out_shift)


# ---- fwrite_write_kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["body", "raw"])
def test_fasta_write_past_the_grid(ctx, which):
    from tests import test_fasta_write_gpu as unit
    case = G.write_cases()[which]
    for out_shift in (0, 7):
        unit.run_case(ctx, case.moved("%s at %d" % (case.name, out_shift), out_shift=out_shift, body_shift=out_shift // 2))


# ---- sketch_long_kernel: the work-sharing shapes of long_block -----------------------------------------------------------------
def check_sketch(ctx, distinct, order, k, log2_bins, seed=0, **place):
    """The batch distinct[order] on the device against the yardstick's answer per distinct record: rows, counts, the total."""
    from tests import sketch_sets
    from tests import test_sketch_gpu as unit
    exp_rows, exp_counts = sketch_sets.expected(tuple(distinct), k, log2_bins, seed)
    rows_want, counts_want = G.replicated(exp_rows, order), G.replicated(exp_counts, order)
    b = unit.Buffers(*sketch_sets.pack([distinct[i] for i in order]), log2_bins, **place)
    b.launch(ctx, k, seed)
    rc, valid, unprocessed = unit.status(ctx)
    rows, counts = b.result()
    assert (rc, valid, unprocessed) == (OK, int(counts_want.astype(np.int64).sum()), 0)
    assert np.array_equal(counts, counts_want)
    assert np.array_equal(rows, rows_want)


@pytest.mark.parametrize("name", G.LONG_CASES)
def test_sketch_long_shapes(ctx, name):
    """leftover_*: n_long < grid with workgroups left over; two_entries: LONG_GRID + 5 long records among 1000 short ones;
    grid_exact: LONG_GRID long records, four of 10 spans with an N on either side of span boundaries 4 and 8; parts_one: 1100 long
    records, 948 idle workgroups, waves that run two spans in a row."""
    k = G.LONG_CASES.index(name)
    check_sketch(ctx, G.long_pool(), G.long_case(name), G.LONG_K, G.LONG_LOG2_BINS, seed=k % 2 * 0x9E3779B97F4A7C15, in_shift=(5 * k) % 16, lead=k)


# ---- sketch_short_kernel -----------------------------------------------------------------------------------------------------
def test_sketch_short_past_the_grid(ctx):
    """40 000 records on SHORT_MAX_GRID workgroups at the largest LDS slice: a wave meets short, empty and long records in turn."""
    distinct, order = G.short_set()
    check_sketch(ctx, distinct, order, G.SHORT_K, G.SHORT_LOG2_BINS, in_shift=3)


# ---- sketch_compare_kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2_bins", [4, 8])
def test_sketch_compare_past_the_grid(ctx, log2_bins):
    from tests import sketch_ref
    from tests import test_sketch_gpu as unit
    a, b, pairs = G.compare_set(log2_bins)
    match, filled, rc, bad = unit.run_compare(ctx, a, b, pairs)
    m, f, exp_bad = sketch_ref.compare_pairs(a, b, pairs)
    assert bad == exp_bad > 100 and rc == INVALID_ARG and (m > 0).mean() > 0.5
    assert np.array_equal(match, m) and np.array_equal(filled, f)
