"""Inputs that carry every fixed-grid kernel past its grid, shared by tests/test_grid_sets_cpu.py (which computes from the sources'
constants that each input reaches its path) and tests/test_grid_stride_gpu.py (which runs them).  TEST INFRASTRUCTURE ONLY.
Everything is seeded; the sizes follow the launch constants read from the sources, so a retune moves the inputs with it."""
import functools
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circkit_amd", "csrc")


# ---- the launch constants ----------------------------------------------------------------------------------------------------
def _value(src, name):
    """The value of `constexpr .. name = expression` in src; the expression may name other constants of the same source."""
    m = re.search(r"constexpr[^;]*?\b%s\s*=(?!=)\s*([^,;]+)[,;]" % name, src)
    assert m, name
    expr = re.sub(r"\b(\d+)(?:ull|ul|u)\b", r"\1", m.group(1))
    expr = re.sub(r"\([a-z0-9_ ]+\)(?=\s*[A-Za-z_(])", "", expr)                  # a cast
    expr = re.sub(r"[A-Za-z_]\w*", lambda t: str(_value(src, t.group(0))), expr)
    assert re.fullmatch(r"[\d\s*+\-<()]+", expr), (name, expr)
    return int(eval(expr))                                                        # digits, * + - << and parentheses only


def _src(name):
    return open(os.path.join(CSRC, name)).read()


@functools.lru_cache(maxsize=None)
def grid_constants():
    c = {}
    c["FASTA_GRID"] = _value(_src("circkit_fasta.hip"), "FASTA_GRID")
    c["FASTA_TILE_BYTES"] = _value(_src("fasta_device.h"), "TILE_BYTES")
    c["COMPACT_GATHER_GRID"] = _value(_src("circkit_monomerize.hip"), "GATHER_GRID")
    c["COMPACT_TILE_BYTES"] = _value(_src("monomer_compact.h"), "TILE_BYTES")
    c["WINDOWS_GATHER_GRID"] = _value(_src("circkit_windows.hip"), "GATHER_GRID")
    c["WINDOWS_TILE_BYTES"] = _value(_src("window_gather.h"), "TILE_BYTES")
    c["TILE_RESIDUES"] = _value(_src("window_translate.h"), "TILE_RESIDUES")
    c["WRITE_GRID"] = _value(_src("circkit_fasta_write.hip"), "WRITE_GRID")
    c["WRITE_TILE_BYTES"] = _value(_src("fasta_write.h"), "TILE_BYTES")
    for name in ("LONG_GRID", "SHORT_MAX_GRID", "COMPARE_MAX_GRID", "COMPARE_WAVES"):
        c[name] = _value(_src("circkit_sketch.hip"), name)
    for name in ("SKETCH_SEG", "SKETCH_WAVES"):
        c[name] = _value(_src("sketch.h"), name)
    return c


def trips(work_units, grid):
    """The trips of the busiest workgroup of `for (t = blockIdx.x; t < work_units; t += gridDim.x)`: workgroup 0's."""
    return -(-int(work_units) // int(grid))


def long_trips(lengths, grid, seg=None, waves=None):
    """sketch.h's long_block restated: `lengths` are the long records in the order of the list.  Returns (the most spans one
    wave runs, the most list entries one workgroup runs, the workgroups left without a record)."""
    c = grid_constants()
    seg, waves = seg or c["SKETCH_SEG"], waves or c["SKETCH_WAVES"]
    n_long = len(lengths)
    most_spans = most_entries = idle = 0
    if n_long == 0:
        return 0, 0, grid
    for block in range(grid):
        e, e_step, part, parts = block, grid, 0, 1
        if n_long < grid:
            parts = grid // n_long
            e, part, e_step = block // parts, block % parts, n_long
        entries = list(range(e, n_long, e_step))
        most_entries = max(most_entries, len(entries))
        idle += not entries
        for w in range(waves):
            spans = sum(len(range(part * waves + w, -(-int(lengths[x]) // seg), parts * waves)) for x in entries)
            most_spans = max(most_spans, spans)
    return most_spans, most_entries, idle


def replicated(distinct, order):
    """The answer for a batch that repeats a few distinct records, record k being distinct record order[k]: the yardstick's
    answer per distinct record (an array with one row per record, or a list of byte strings) indexed by `order`."""
    order = np.asarray(order, dtype=np.int64)
    if isinstance(distinct, np.ndarray):
        return distinct[order]
    return b"".join(distinct[i] for i in order)


def _acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(n))].tobytes()


# ---- FASTA parse -------------------------------------------------------------------------------------------------------------
def _wrapped(seq, eol, width=70):
    return b"".join(seq[a:a + width] + eol for a in range(0, len(seq), width))


@functools.lru_cache(maxsize=None)
def fasta_text():
    """(text, marks): wrapped 1 kb records over 2 * FASTA_GRID + 3 tiles, so that workgroups 0..2 make three trips, with these
    laid in (marks names the positions):
      start_last   a record start on the last byte of tile FASTA_GRID - 1, whose header covers tile FASTA_GRID whole (that
                   workgroup's second tile is ST_PASS) and ends in tile FASTA_GRID + 1
      start_first  a record start on the first byte of tile FASTA_GRID + 3 (tile FASTA_GRID itself lies inside the header)
      blank        a run of '\\n', ' ', '\\t', '\\r' over tile FASTA_GRID + 5 whole: a second trip that keeps nothing
      crlf         a stretch of records with CRLF line ends
      poly         one line of one base from inside tile 2 * FASTA_GRID - 1 to inside tile 2 * FASTA_GRID + 1
    The text ends in the middle of a line."""
    c = grid_constants()
    G, T = c["FASTA_GRID"], c["FASTA_TILE_BYTES"]
    rng = np.random.default_rng(1601)
    pool = _acgt(rng, 1 << 20)
    out, marks, count = bytearray(), {}, [0]

    def record(eol=b"\n"):
        at = int(rng.integers(0, len(pool) - 1000))
        count[0] += 1
        return b">r%d some text" % count[0] + eol + _wrapped(pool[at:at + 1000], eol)

    def fill_to(pos):
        """Records up to `pos` exactly: the last one is a single line sized to end there."""
        while len(out) + 2300 < pos:
            out.extend(record())
        gap = pos - len(out)
        assert gap >= 8
        out.extend(b">p\n" + b"G" * (gap - 4) + b"\n")

    fill_to(G * T - 1)
    marks["start_last"] = len(out)
    out.extend(b">" + b"h" * (T + 300) + b" tail\n" + _wrapped(pool[:500], b"\n"))
    fill_to((G + 3) * T)
    marks["start_first"] = len(out)
    out.extend(record())
    fill_to((G + 5) * T - 7)
    out.extend(b">w\nAC")
    marks["blank"] = len(out)
    out.extend((b"\n \t\r" * (T // 4 + 8))[:T + 20] + b"\nGT\n")
    marks["blank_end"] = marks["blank"] + T + 20
    marks["crlf"] = len(out)
    for _ in range(24):
        out.extend(record(b"\r\n"))
    marks["crlf_end"] = len(out)
    fill_to((2 * G - 1) * T + 100 - 6)
    out.extend(b">poly\n")
    marks["poly"] = len(out)
    out.extend(b"A" * (2 * T) + b"\n")
    marks["poly_end"] = marks["poly"] + 2 * T
    total = (2 * G + 3) * T - 5
    while len(out) < total + 40:
        out.extend(record())
    return bytes(out[:total]), marks


# ---- the two compacts --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compact_batch():
    """(data, offsets, keep): 36 000 records of 1 kb drawn from 600 distinct ones with one 3 MB record in the middle; the seeded
    mask keeps the big record and as many others as bring the kept payload to GATHER_GRID + 5 tiles + 77 bytes or a little more."""
    c = grid_constants()
    want = (c["COMPACT_GATHER_GRID"] + 5) * c["COMPACT_TILE_BYTES"] + 77
    rng = np.random.default_rng(1602)
    n, size, big = 36_000, 1000, 3_000_000
    pool = rng.integers(0, 256, size=(600, size), dtype=np.uint8)
    order = rng.integers(0, 600, size=n)
    data = np.concatenate([pool[order[:n // 2]].reshape(-1), rng.integers(0, 256, size=big, dtype=np.uint8), pool[order[n // 2:]].reshape(-1)])
    lengths = np.full(n + 1, size, dtype=np.int64)
    lengths[n // 2] = big
    offs = np.zeros(n + 2, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    n_keep = -(-(want - big) // size)
    assert 0 < n_keep < n
    keep = np.zeros(n + 1, dtype=bool)
    small = np.delete(np.arange(n + 1), n // 2)
    keep[rng.permutation(small)[:n_keep]] = True
    keep[n // 2] = True
    return data, offs, keep


def compact_ends(offs, keep):
    """The crafted end indices of the monomer compact: a kept record is written whole, the others have no monomer."""
    return np.where(keep, np.diff(offs.astype(np.int64)), 0xFFFFFFFF).astype(np.uint32)


def compact_first_seen(keep):
    """The crafted first_seen of the uniq compact: a kept record is its own first, a dropped one names an earlier record or ~0."""
    rng = np.random.default_rng(1603)
    i = np.arange(len(keep), dtype=np.uint64)
    earlier = (rng.random(len(keep)) * i).astype(np.uint64)                         # < i from record 1 on
    drop = np.where((rng.random(len(keep)) < 0.5) & (i > 0), earlier, np.uint64(2 ** 64 - 1))
    return np.where(keep, i, drop).astype(np.uint64)


# ---- windows: gather and translate -------------------------------------------------------------------------------------------
N_LONG_WINDOWS, N_SMALL_WINDOWS = 60, 20_000
WRAP = 2 ** 32 - 1


def _windows_layout(lengths, grid, tile, unit, seed):
    """The window list of either large set over records of `lengths`, in output units of `unit` symbols (1: bytes, 3: residues):
    17 000 small windows (1..40 units), the 60 long ones, 1 500 small ones that straddle output unit grid * tile, one window
    that tops the output up to just past grid + 3 tiles, 1 500 small ones; invalid windows between the blocks.  Returns
    (windows, segments): segments = [(kind, first window, one past the last)], kind "small" (invalid ones included) or "long"."""
    from tests.windows_ref import WINDOW_DTYPE
    from tests.windows_sets import invalid_rows
    rng = np.random.default_rng(seed)
    nr = len(lengths)
    real = [r for r, n in enumerate(lengths) if n > 0]

    def small(count):
        w = np.zeros(count, dtype=WINDOW_DTYPE)
        w["length"] = unit * rng.integers(1, 41, size=count) + (rng.integers(0, unit, size=count) if unit > 1 else 0)
        w["record"] = np.array(real)[rng.integers(0, len(real), size=count)]
        w["start"] = rng.integers(0, 2 ** 32, size=count)
        w["strand"] = rng.integers(0, 2, size=count)
        return w

    def invalid(rows):
        w = np.zeros(len(rows), dtype=WINDOW_DTYPE)
        for k, r in enumerate(rows):
            w[k] = tuple(r) + (0,) * (5 - len(r))
        return w

    units = lambda w: int((w["length"] // np.uint64(unit)).sum())
    bad = invalid_rows(nr)
    a, b, c = small(17_000), small(1_500), small(1_500)
    # the long ones end where half of block b is still to come before output unit grid * tile
    long_total = grid * tile - units(a) - units(b) // 2
    base = long_total // N_LONG_WINDOWS
    long = np.zeros(N_LONG_WINDOWS, dtype=WINDOW_DTYPE)
    for k in range(N_LONG_WINDOWS):
        r = real[k % len(real)]
        n = lengths[r]
        span = base + (long_total - base * N_LONG_WINDOWS if k == 0 else 0)
        long[k] = (unit * span + (k % unit), r, (0, n - 1, n + 7, WRAP)[(k // len(real)) % 4], k & 1, 0)
    top = (grid + 3) * tile + 101 - (units(a) + long_total + units(b) + units(c))
    assert 0 < top < tile
    top_up = invalid([(unit * top, real[-1], 5, 1)])
    parts = [("small", a), ("small", invalid(bad[:2]))] + [("long", long[k:k + 1]) for k in range(N_LONG_WINDOWS)] + \
        [("small", invalid(bad[2:])), ("small", b), ("small", invalid(bad[:1])), ("small", top_up), ("small", c), ("small", invalid(bad[1:3]))]
    wins = np.concatenate([p for _, p in parts])
    segments, at = [], 0
    for kind, p in parts:
        if segments and kind == "small" and segments[-1][0] == "small":
            segments[-1] = ("small", segments[-1][1], at + len(p))
        else:
            segments.append((kind, at, at + len(p)))
        at += len(p)
    return wins, segments


def _gather_lengths():
    """windows_sets.RECORD_LENGTHS and five more, up to 5000 symbols: 16 lengths."""
    from tests.windows_sets import RECORD_LENGTHS
    return list(RECORD_LENGTHS) + [5, 333, 2500, 4999, 5000]


@functools.lru_cache(maxsize=None)
def gather_set():
    """(data, offsets, windows, segments) of the large gather: 16 record lengths, 0 to 5000 symbols."""
    from tests import windows_sets
    c = grid_constants()
    data, offs = windows_sets.batch(np.random.default_rng(1604), _gather_lengths())
    wins, segments = _windows_layout(_gather_lengths(), c["WINDOWS_GATHER_GRID"], c["WINDOWS_TILE_BYTES"], 1, 1605)
    return data, offs, wins, segments


def _translate_lengths():
    from tests.translate_sets import RECORD_LENGTHS
    return list(RECORD_LENGTHS) + [5000]


@functools.lru_cache(maxsize=None)
def translate_set():
    """(data, offsets, windows, segments) of the large translate: the same shape in residues; records of 1 and of 2 symbols are
    among the long windows' (every codon of those crosses the origin)."""
    from tests import translate_sets
    c = grid_constants()
    data, offs = translate_sets.batch(np.random.default_rng(1606), _translate_lengths())
    wins, segments = _windows_layout(_translate_lengths(), c["WINDOWS_GATHER_GRID"], c["TILE_RESIDUES"], 3, 1607)
    return data, offs, wins, segments


def periodic_protein(record, start, strand, n_residues, aa, unknown=b"X"):
    """The protein of a window of n_residues codons on `record` (n symbols) from `start` on `strand`.  Codon t starts at
    (start + 3t) mod n, so codon t + n is codon t: the first min(n_residues, n) codons are translated plainly
    (translate_ref.translate over the bytes windows_ref.gather cuts) and that period is repeated to length."""
    from tests import translate_ref, windows_ref
    record = bytes(record)
    n = len(record)
    if n == 0 or n_residues <= 0:
        return b""
    period = min(int(n_residues), n)
    w = windows_ref.windows([(3 * period, 0, int(start), int(strand))])
    cut, _, bad = windows_ref.gather(np.frombuffer(record, dtype=np.uint8), np.array([0, n], dtype=np.uint64), w)
    assert bad == 0 and len(cut) == 3 * period
    head = translate_ref.translate(bytes(cut), aa, unknown)
    return (head * (-(-int(n_residues) // period)))[:int(n_residues)]


def translate_expected(data, offs, wins, segments, aa, unknown=b"X"):
    """(aa_bytes, aa_offsets, n_invalid) of the large translate: a long window by periodic_protein, a run of small and invalid
    ones by translate_ref.windows_translate on its own slice."""
    from tests import translate_ref
    raw, o = bytes(data), [int(x) for x in offs]
    parts, counts, bad = [], [], 0
    for kind, lo, hi in segments:
        if kind == "long":
            w = wins[lo]
            r = int(w["record"])
            parts.append(periodic_protein(raw[o[r]:o[r + 1]], w["start"], w["strand"], int(w["length"]) // 3, aa, unknown))
            counts.append(np.array([len(parts[-1])], dtype=np.int64))
        else:
            out, off, b = translate_ref.windows_translate(data, offs, wins[lo:hi], aa, unknown)
            parts.append(out.tobytes())
            counts.append(np.diff(off.astype(np.int64)))
            bad += b
    aa_off = np.zeros(len(wins) + 1, dtype=np.uint64)
    aa_off[1:] = np.cumsum(np.concatenate(counts))
    return np.frombuffer(b"".join(parts), dtype=np.uint8), aa_off, bad


# ---- FASTA write -------------------------------------------------------------------------------------------------------------
N_WRITE = 33_500


@functools.lru_cache(maxsize=None)
def write_cases():
    """(body case, raw case): 33 500 output records whose heads come from a parsed text of 500 records of 1 kb through a
    d_out_src map.  The body case takes bodies of about 1 kb from a CSR batch, sized so that the total is just past
    WRITE_GRID + 2 tiles, and labels (the ABI labels every output or none: every third is on the reverse strand); the raw case
    writes the raw spans of the text instead and has no labels."""
    from tests import fasta_sets, fasta_write_sets as W
    c = grid_constants()
    rng = np.random.default_rng(1608)
    text = fasta_sets.records_text(rng, 500, 1000, width=70)
    parsed = fasta_sets.host(text)
    assert parsed["records"] == 500
    head, raw = parsed["head"].copy(), parsed["raw"].copy()
    src = rng.integers(0, 500, size=N_WRITE).astype(np.uint64)
    labels = np.zeros(N_WRITE, dtype=W.WINDOW_DTYPE)
    labels["length"] = 77
    labels["record"] = np.arange(N_WRITE)
    labels["start"] = np.array(W.LABEL_STARTS, dtype=np.uint64)[rng.integers(0, len(W.LABEL_STARTS), size=N_WRITE)]
    labels["strand"] = np.arange(N_WRITE) % 3 == 2
    fixed = sum(3 + int(head[int(h)][1]) + len(W.label_of(int(s), int(p))) for h, s, p in zip(src, labels["strand"], labels["start"]))
    size = ((c["WRITE_GRID"] + 2) * c["WRITE_TILE_BYTES"] - fixed) // N_WRITE + 1
    assert 900 <= size <= 1100, size
    body = np.frombuffer(b"ACGTN", dtype=np.uint8)[rng.integers(0, 5, size=N_WRITE * size)]
    offs = size * np.arange(N_WRITE + 1, dtype=np.uint64)
    return (W.Case("past_the_grid_body", text, head, body=body.tobytes(), offsets=offs, src=src, labels=labels),
            W.Case("past_the_grid_raw", text, head, raw=raw, src=src))


# ---- sketch ------------------------------------------------------------------------------------------------------------------
LONG_K, LONG_LOG2_BINS = 21, 8
SHORT_K, SHORT_LOG2_BINS = 32, 10
N_LONG_POOL = 12
LONG_CASES = ("leftover_3", "leftover_5", "leftover_700", "two_entries", "grid_exact", "parts_one")
# what each case claims: spans per wave >= 2, list entries per workgroup >= 2, workgroups left over > 0
LONG_CLAIMS = {"leftover_3": (False, False, True), "leftover_5": (False, False, True), "leftover_700": (False, False, True),
               "two_entries": (True, True, False), "grid_exact": (True, False, False), "parts_one": (True, False, True)}


@functools.lru_cache(maxsize=None)
def long_pool():
    """The distinct records of the long-kernel cases: 12 long ones (about 130 000 k-mers in all) and 10 short ones."""
    from tests.sketch_sets import with_symbol
    seg = grid_constants()["SKETCH_SEG"]
    rng = np.random.default_rng(1609)
    lens = [seg + 1, seg + 2, seg + 20, seg + 39, seg + 40, 2 * seg, 2 * seg + 1, 3 * seg + 5, 4 * seg + 10, 9 * seg + 5, seg + 7, 5 * seg]
    long = [_acgt(rng, n) for n in lens]
    long[7] = with_symbol(long[7], [0, seg - 1, 3 * seg + 4])
    long[9] = with_symbol(long[9], [4 * seg - 1, 4 * seg, 8 * seg - 1, 8 * seg])       # an N on either side of span boundaries 4 and 8
    long[10] = with_symbol(long[10], [seg, seg + 6], b"n")
    short = [_acgt(rng, n) for n in (0, 20, 21, 30, 64, 333, 1000, seg - 1, seg)] + [with_symbol(_acgt(rng, 500), [77, 250])]
    assert len(long) == N_LONG_POOL
    return tuple(long + short)


def _interleave(rng, long_ids, short_ids):
    """The long records in order with the short ones spread evenly between them."""
    n = len(long_ids) + len(short_ids)
    is_short = np.zeros(n, dtype=bool)
    if len(short_ids):
        is_short[np.linspace(0, n - 1, len(short_ids)).astype(np.int64)] = True
    assert int(is_short.sum()) == len(short_ids)
    order = np.empty(n, dtype=np.int64)
    order[is_short], order[~is_short] = short_ids, long_ids
    return order


@functools.lru_cache(maxsize=None)
def long_case(name):
    """The record order (indices into long_pool()) of one long-kernel case."""
    c = grid_constants()
    grid, P = c["LONG_GRID"], N_LONG_POOL
    rng = np.random.default_rng(1610 + LONG_CASES.index(name))
    shorts = lambda count: P + rng.integers(0, 10, size=count)
    if name.startswith("leftover_"):
        n_long = int(name.split("_")[1])
        ids = rng.integers(0, P, size=n_long)
        ids[ids == 9] = 8                                                         # the 10-span record: in leftover_3 only
        if n_long == 3:
            ids[:] = (9, 0, 6)
        return _interleave(rng, ids, shorts(50))
    if name == "two_entries":
        return _interleave(rng, rng.integers(0, 5, size=grid + 5), shorts(1000))   # seg + 1 .. seg + 40 symbols
    if name == "grid_exact":
        ids = rng.integers(0, 8, size=grid)
        ids[[0, grid // 3, grid // 2, grid - 1]] = 9
        return ids.astype(np.int64)
    if name == "parts_one":
        ids = rng.integers(0, 8, size=1100)
        ids[[7, 1000]] = (8, 11)
        return _interleave(rng, ids, shorts(30))
    raise KeyError(name)


def long_lengths(name):
    """The lengths of the case's long records in the order of the batch (the device's list holds them in some order)."""
    pool, seg = long_pool(), grid_constants()["SKETCH_SEG"]
    return [len(pool[i]) for i in long_case(name) if len(pool[i]) > seg]


@functools.lru_cache(maxsize=None)
def short_set():
    """(distinct, order): 40 000 records drawn from 300 distinct ones of 0, k - 1, k, 30, 333, SEG - 1 and SEG symbols, with 40
    copies of one record of SEG + 1 symbols spread evenly."""
    from tests.sketch_sets import with_symbol
    seg, k = grid_constants()["SKETCH_SEG"], SHORT_K
    rng = np.random.default_rng(1620)
    lens = [0] + [k - 1] * 5 + [k] * 5 + [30] * 140 + [333] * 140 + [seg - 1] * 4 + [seg] * 4
    distinct = [_acgt(rng, n) for n in lens]
    distinct[20] = with_symbol(distinct[20], [3])
    distinct[200] = with_symbol(distinct[200], [0, 100, 332])
    distinct.append(_acgt(rng, seg + 1))
    assert len(distinct) == 300
    order = rng.integers(0, 299, size=40_000)
    order[np.linspace(17, 39_990, 40).astype(np.int64)] = 299
    return tuple(distinct), order


N_COMPARE_A, N_COMPARE_B = 300, 200


@functools.lru_cache(maxsize=None)
def compare_set(log2_bins):
    """(rows a, rows b, pairs): COMPARE_MAX_GRID * COMPARE_WAVES + 1000 pairs over 300 x 200 rows.  The bins hold one of four
    values spread over the whole 64-bit range, the top bit included, or EMPTY, so that many bins match by chance; about 0.1 % of
    the pairs name a row that does not exist."""
    c = grid_constants()
    rng = np.random.default_rng(1630 + log2_bins)
    bins = 1 << log2_bins
    palette = np.array([1, 2 ** 63, 2 ** 64 - 2, 0x8000000000000001], dtype=np.uint64)
    a = palette[rng.integers(0, 4, size=(N_COMPARE_A, bins))]
    b = palette[rng.integers(0, 4, size=(N_COMPARE_B, bins))]
    a[rng.random(a.shape) < 0.2] = np.uint64(2 ** 64 - 1)
    b[rng.random(b.shape) < 0.2] = np.uint64(2 ** 64 - 1)
    m = c["COMPARE_MAX_GRID"] * c["COMPARE_WAVES"] + 1000
    pairs = np.stack([rng.integers(0, N_COMPARE_A, size=m), rng.integers(0, N_COMPARE_B, size=m)], axis=1).astype(np.uint32)
    bad = np.flatnonzero(rng.random(m) < 0.001)
    pairs[bad[0::3], 0] = N_COMPARE_A
    pairs[bad[1::3], 1] = N_COMPARE_B
    pairs[bad[2::3]] = 2 ** 32 - 1
    pairs[-1] = (N_COMPARE_A - 1, N_COMPARE_B)                                     # the last pair of the second trip is invalid
    return a, b, pairs
