"""GPU: circkit_sketch_batch_device / _status / circkit_sketch_compare_device / _status and the host forms against the yardstick
tests/sketch_ref.py, exactly: every bin, every count, every (match, filled).  The input sets are tests/sketch_sets.py's, the ones
the CPU fiber test runs; canaries surround the payload, the rows and the counts."""
import ctypes

import numpy as np
import pytest

from tests import sketch_ref as R
from tests import sketch_sets as S

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY = 0x4E
ROW_CANARY, COUNT_CANARY = 0x25A5A5A5A5A5A5A5, 0x3F3F3F3F
OK, INVALID_ARG, TOO_LONG = 0, -1, -4
SEG = S.constants()["SKETCH_SEG"]
EMPTY = np.uint64(R.EMPTY)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    """A ctx that launches on torch's current stream, so that the tensors torch fills and the ctx's kernels are ordered."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def status(ctx):
    """(rc, valid k-mers, unprocessed records) of the last sketch, without raising."""
    t, bad = ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = ctx._lib.circkit_sketch_status(ctx._h, ctypes.byref(t), ctypes.byref(bad))
    return rc, t.value, bad.value


def compare_status(ctx):
    bad = ctypes.c_uint64(0)
    rc = ctx._lib.circkit_sketch_compare_status(ctx._h, ctypes.byref(bad))
    return rc, bad.value


class Buffers:
    """A batch on the device: the payload at in_shift mod 16 behind `lead` canary bytes (offsets[0] = lead), canaries round the
    payload, the rows and the counts."""

    def __init__(self, data, offs, log2_bins, in_shift=0, lead=0, counts=True):
        import torch
        self.n, self.bins, self.log2_bins = len(offs) - 1, 1 << log2_bins, log2_bins
        nb = len(data)
        raw = np.full(GUARD + in_shift + lead + nb + GUARD, IN_CANARY, dtype=np.uint8)
        raw[GUARD + in_shift + lead:GUARD + in_shift + lead + nb] = data
        self.raw_in = raw
        self.d_raw = _to(raw)
        self.d_bytes = self.d_raw[GUARD + in_shift:]
        self.offs = np.asarray(offs, dtype=np.uint64) + np.uint64(lead)
        self.d_offs = _to(_i64(self.offs))
        self.d_rows = torch.full((GUARD + self.n * self.bins + GUARD,), ROW_CANARY, dtype=torch.int64, device=_dev())
        self.d_counts = torch.full((GUARD + self.n + GUARD,), COUNT_CANARY, dtype=torch.int32, device=_dev())
        self.want_counts = counts
        assert self.d_bytes.data_ptr() % 16 == in_shift % 16

    def launch(self, ctx, k, seed=0):
        ctx.sketch_batch_device(self.d_bytes, self.d_offs, self.n, self.d_rows[GUARD:], self.d_counts[GUARD:] if self.want_counts else None,
                                k=k, log2_bins=self.log2_bins, seed=seed)

    def result(self):
        """(rows, counts) after the canary checks."""
        rows, counts = self.d_rows.cpu().numpy().view(np.uint64), self.d_counts.cpu().numpy().view(np.uint32)
        assert np.array_equal(self.d_raw.cpu().numpy(), self.raw_in), "the sketch wrote into its input"
        assert np.array_equal(self.d_offs.cpu().numpy().view(np.uint64), self.offs), "the sketch wrote into the offsets"
        assert (rows[:GUARD] == ROW_CANARY).all() and (rows[GUARD + self.n * self.bins:] == ROW_CANARY).all(), "rows written outside the n records'"
        assert (counts[:GUARD] == COUNT_CANARY).all() and (counts[GUARD + self.n:] == COUNT_CANARY).all(), "counts written outside the n records'"
        if not self.want_counts:
            assert (counts == COUNT_CANARY).all()
        return rows[GUARD:GUARD + self.n * self.bins].reshape(self.n, self.bins).copy(), counts[GUARD:GUARD + self.n].copy()


def check(ctx, records, k, log2_bins, seed=0, what="", **place):
    records = tuple(records)
    exp_rows, exp_counts = S.expected(records, k, log2_bins, seed)
    b = Buffers(*S.pack(records), log2_bins, **place)
    b.launch(ctx, k, seed)
    rc, valid, unprocessed = status(ctx)
    rows, counts = b.result()
    assert (rc, valid, unprocessed) == (OK, int(exp_counts.sum()), 0), (what, rc, valid, unprocessed)
    if b.want_counts:
        assert np.array_equal(counts, exp_counts), what
    assert np.array_equal(rows, exp_rows), what
    return rows, counts


# ---- 1. lengths, k, bins, alignments -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(S.PARAMS)), ids=["k%d-bins%d" % (k, 1 << b) for k, b in S.PARAMS])
def test_every_length(ctx, i):
    """Every length 0 .. 200, round 256 and 1024, round SKETCH_SEG and its multiples, and k - 1, k, k + 1."""
    k, b = S.PARAMS[i]
    assert {k - 1, k, k + 1, SEG - 1, SEG, SEG + 1, 2 * SEG, 2 * SEG + 1, 3 * SEG + k - 2} <= set(S.lengths(k))
    check(ctx, S.length_records(k), k, b, seed=i % 2 * 0x9E3779B97F4A7C15, what=(k, b), in_shift=(5 * i) % 16, lead=3 * i + 1)


def test_every_alignment_of_the_payload(ctx):
    recs = S.length_records(21)[150:]                                           # 150 .. 200 and everything longer
    for shift in range(16):
        check(ctx, recs, 21, 6, seed=shift, what=shift, in_shift=shift, lead=shift % 3, counts=shift != 7)


# ---- 2. symbols ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,b,seed", ((21, 8, 0), (4, 4, 5), (32, 6, 2 ** 64 - 1), (16, 10, 1)))
def test_symbols(ctx, k, b, seed):
    """An N at each of the 40 positions of a record, all N, '-', lower case, other bytes, invalid symbols on either side of a span
    boundary, poly-A (c = 0), palindromic k-mers (f == r), under more than one seed."""
    named = S.symbol_records(k)
    rows, counts = check(ctx, [s for _, s in named], k, b, seed, what=(k, b, seed), in_shift=3, lead=1)
    got = dict(zip([n for n, _ in named], counts))
    assert got["all N"] == got["lower case"] == 0 and got["poly-A"] == 100
    assert all(got["N at %d" % p] == max(40 - k, 0) for p in range(40))


def test_the_hash_that_equals_empty(ctx):
    """A poly-A record under the seed that sends its one canonical k-mer to 2^64 - 1: the row is all EMPTY, the k-mers are counted."""
    seed = S.poly_a_seed_for_empty(21)
    assert R.fmix64(seed) == R.EMPTY
    recs = (b"A" * 100, b"T" * 30, b"A" * (SEG + 9), b"ACGT" * 20)
    rows, counts = check(ctx, recs, 21, 8, seed, what="h = EMPTY")
    assert (rows[:3] == EMPTY).all() and counts.tolist()[:3] == [100, 30, SEG + 9] and (rows[3] != EMPTY).any()


# ---- 3. invariance through the project's own device calls ----------------------------------------------------------------------
def invariance_records():
    rng = np.random.default_rng(21)
    lens = [21, 22, 64, 333, 1000, SEG - 1, SEG, SEG + 1, 2 * SEG + 77]
    return tuple(S.with_symbol(S.random_acgt(rng, n), [n // 3] if i % 3 == 1 else []) for i, n in enumerate(lens))


def test_the_row_is_invariant(ctx):
    """rotate_batch, revcomp_batch, cat_batch and canonicalize_batch_device of a batch sketch to the same rows, bit for bit, for
    lengths on both sides of SKETCH_SEG (cat: the counts double)."""
    import torch
    recs = invariance_records()
    data, offs = S.pack(recs)
    rows, counts = check(ctx, recs, 21, 8, seed=3, what="base")
    for name, (d2, o2), factor in (("rotate", ctx.rotate_batch(data, offs, bases=17), 1), ("rotate %", ctx.rotate_batch(data, offs, percent=0.37), 1),
                                   ("revcomp", ctx.revcomp_batch(data, offs), 1), ("cat", ctx.cat_batch(data, offs), 2)):
        assert not np.array_equal(d2, data), name
        b = Buffers(d2, o2, 8, in_shift=5)
        b.launch(ctx, 21, 3)
        assert status(ctx)[0] == OK
        r2, c2 = b.result()
        assert np.array_equal(r2, rows), name
        assert np.array_equal(c2, counts * factor), name
    # the canonical form, on the device from end to end
    b = Buffers(data, offs, 8)
    d_canon = torch.zeros(len(data) + 64, dtype=torch.uint8, device=_dev())
    ctx.canonicalize_batch_device(b.d_bytes, b.d_offs, b.n, out_bytes=d_canon)
    assert ctx.batch_status() == 0
    ctx.sketch_batch_device(d_canon, b.d_offs, b.n, b.d_rows[GUARD:], b.d_counts[GUARD:], k=21, log2_bins=8, seed=3)
    assert status(ctx)[0] == OK
    r2, c2 = b.result()
    assert not np.array_equal(d_canon.cpu().numpy()[:len(data)], data)
    assert np.array_equal(r2, rows) and np.array_equal(c2, counts)


# ---- 4. scale that only the card runs ------------------------------------------------------------------------------------------
def test_seventy_thousand_short_records(ctx):
    rng = np.random.default_rng(70)
    distinct = tuple(S.random_acgt(rng, 30) for _ in range(700))
    exp_rows, exp_counts = S.expected(distinct, 21, 4)
    order = rng.integers(0, 700, size=70_000)
    b = Buffers(*S.pack([distinct[i] for i in order]), 4, in_shift=9)
    b.launch(ctx, 21)
    rc, valid, unprocessed = status(ctx)
    rows, counts = b.result()
    assert (rc, valid, unprocessed) == (OK, 70_000 * 30, 0)
    assert np.array_equal(rows, exp_rows[order]) and np.array_equal(counts, exp_counts[order])


def test_no_records(ctx):
    b = Buffers(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), 8)
    b.launch(ctx, 21)
    assert status(ctx) == (OK, 0, 0)
    b.result()
    assert ctx._lib.circkit_sketch_batch_device(ctx._h, None, None, 0, ctypes.byref(__import__("circkit_amd").sketch_params()), None, None) == OK
    assert status(ctx) == (OK, 0, 0)


def test_one_very_long_record_among_short_ones(ctx):
    rng = np.random.default_rng(40)
    recs = [S.random_acgt(rng, n) for n in (100, 30, 40 * SEG, 1000, SEG + 1, 5)]
    recs[2] = S.with_symbol(recs[2], [0, 7 * SEG - 1, 7 * SEG, 40 * SEG - 1])
    check(ctx, recs, 21, 8, seed=1, what="40 spans", in_shift=1, lead=7)


def test_two_sketches_back_to_back(ctx):
    """Nothing waits between the two; each output is its own sketch's, the status is the second's, and a repeat gives the same bits."""
    recs = S.length_records(21)[180:]
    data, offs = S.pack(recs)
    a, b, c = Buffers(data, offs, 8), Buffers(data, offs, 6, in_shift=2), Buffers(data, offs, 8, in_shift=11)
    a.launch(ctx, 21, seed=1)
    b.launch(ctx, 16, seed=2)
    rc, valid, _ = status(ctx)
    assert rc == OK and valid == int(S.expected(recs, 16, 6, 2)[1].sum())
    c.launch(ctx, 21, seed=1)
    assert status(ctx)[1] == int(S.expected(recs, 21, 8, 1)[1].sum())
    for buf, (k, lb, seed) in ((a, (21, 8, 1)), (b, (16, 6, 2)), (c, (21, 8, 1))):
        rows, counts = buf.result()
        exp = S.expected(recs, k, lb, seed)
        assert np.array_equal(rows, exp[0]) and np.array_equal(counts, exp[1])


def test_each_status_answers_for_its_own_kind(ctx):
    """A sketch between a gather and its circkit_windows_status, and a compare behind both."""
    import torch
    from circkit_amd import api
    recs = (b"ACGTTGCAAC" * 5, b"GATTACA" * 9)
    data, offs = S.pack(recs)
    wins = np.zeros(2, dtype=api.WINDOW_DTYPE)
    wins["length"], wins["record"] = [50, 63], [0, 1]
    d_bytes, d_offs, d_win = _to(data), _to(_i64(offs)), _to(wins.view(np.uint8))
    d_out, d_out_off = torch.zeros(200, dtype=torch.uint8, device=_dev()), torch.zeros(3, dtype=torch.int64, device=_dev())
    ctx.windows_gather_device(d_bytes, d_offs, 2, d_win, 2, d_out, 200, d_out_off)
    b = Buffers(data, offs, 4)
    b.launch(ctx, 5)
    d_pairs, d_res = _to(np.array([[0, 1], [1, 2]], dtype=np.uint32).view(np.int32)), torch.zeros((2, 2), dtype=torch.int32, device=_dev())
    ctx.sketch_compare_device(b.d_rows[GUARD:], 2, b.d_rows[GUARD:], 2, 4, d_pairs, 2, d_res)
    assert ctx.windows_status() == (113, 0)
    exp = S.expected(recs, 5, 4)
    assert status(ctx) == (OK, int(exp[1].sum()), 0)
    assert compare_status(ctx) == (INVALID_ARG, 1)
    assert ctx.windows_status() == (113, 0) and status(ctx)[1] == int(exp[1].sum())
    assert np.array_equal(b.result()[0], exp[0])
    assert d_res.cpu().numpy().view(np.uint32).tolist() == [list(R.compare(exp[0][0], exp[0][1])), [0, 0]]


def test_a_record_of_2_to_the_31_is_counted_and_not_read(ctx):
    """Crafted offsets: the last record claims 2^31 symbols (or its offsets decrease); it gets an EMPTY row and count 0."""
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    exp = S.expected((b"ACGTACGTAC",), 4, 4)
    for offs in ([0, 10, 10 + 2 ** 31], [0, 10, 4]):
        b = Buffers(data, np.array(offs, dtype=np.uint64), 4, lead=2)
        b.launch(ctx, 4)
        rc, valid, unprocessed = status(ctx)
        rows, counts = b.result()
        assert (rc, valid, unprocessed) == (TOO_LONG, 10, 1)
        assert np.array_equal(rows[0], exp[0][0]) and (rows[1] == EMPTY).all() and counts.tolist() == [10, 0]


# ---- 5. compare ----------------------------------------------------------------------------------------------------------------
def run_compare(ctx, a, other, pairs):
    """(match, filled, rc, n_invalid); other None: the same pointer twice.  Canaries round the result."""
    import torch
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    m, log2_bins = len(pairs), a.shape[1].bit_length() - 1
    d_a = _to(a.view(np.int64))
    d_b = d_a if other is None else _to(other.view(np.int64))
    d_pairs = _to(pairs.view(np.int32)) if m else None
    d_res = torch.full((GUARD + 2 * m + GUARD,), COUNT_CANARY, dtype=torch.int32, device=_dev())
    ctx.sketch_compare_device(d_a, len(a), d_b, len(a) if other is None else len(other), log2_bins, d_pairs, m, d_res[GUARD:])
    rc, bad = compare_status(ctx)
    res = d_res.cpu().numpy().view(np.uint32)
    assert (res[:GUARD] == COUNT_CANARY).all() and (res[GUARD + 2 * m:] == COUNT_CANARY).all(), "results written outside the m pairs'"
    assert np.array_equal(d_a.cpu().numpy().view(np.uint64), a) and (m == 0 or np.array_equal(d_pairs.cpu().numpy().view(np.uint32), pairs))
    res = res[GUARD:GUARD + 2 * m].reshape(m, 2)
    return res[:, 0], res[:, 1], rc, bad


@pytest.mark.parametrize("log2_bins", S.LOG2_BINS)
def test_compare(ctx, log2_bins):
    """Identical, disjoint, empty and half-empty rows; the same pointer and two arrays of different sizes; each kind of invalid
    pair among valid neighbours; no pairs."""
    rng = np.random.default_rng(10 + log2_bins)
    a, other = S.compare_rows(rng, log2_bins), S.compare_rows(rng, log2_bins, n=9)
    other[2] = a[0]
    na, nb, bins = len(a), len(other), 1 << log2_bins
    same_pairs = [(i, j) for i in range(10) for j in range(10)] + [(3, na), (na, 3), (5, 5), (2 ** 32 - 1, 0), (0, 2 ** 32 - 1), (1, 0)]
    diff_pairs = [(i, j) for i in range(na) for j in range(nb)] + [(na, 0), (0, 0), (0, nb), (nb, 2), (2 ** 32 - 1, 2 ** 32 - 1), (0, 2)]
    for x, y, pairs, n_bad in ((a, None, same_pairs, 4), (a, other, diff_pairs, 3), (a, other, [], 0), (a, None, [(0, 1), (3, 4), (0, 3)], 0)):
        match, filled, rc, bad = run_compare(ctx, x, y, pairs)
        m, f, exp_bad = R.compare_pairs(x, x if y is None else y, pairs)
        assert exp_bad == n_bad == bad and rc == (INVALID_ARG if n_bad else OK)
        assert np.array_equal(match, m) and np.array_equal(filled, f)
    assert (match.tolist(), filled.tolist()) == ([bins, 0, 0], [bins, 0, bins])     # identical; both empty; one empty


def test_compare_a_hundred_thousand_pairs(ctx):
    rng = np.random.default_rng(100)
    a = rng.integers(0, 4, size=(300, 16), dtype=np.uint64)                          # few values: many bins match by chance
    a[rng.random(a.shape) < 0.2] = EMPTY
    b = rng.integers(0, 4, size=(200, 16), dtype=np.uint64)
    b[rng.random(b.shape) < 0.2] = EMPTY
    pairs = np.stack([rng.integers(0, 301, size=100_000), rng.integers(0, 201, size=100_000)], axis=1)
    match, filled, rc, bad = run_compare(ctx, a, b, pairs)
    m, f, exp_bad = R.compare_pairs(a, b, pairs)
    assert bad == exp_bad > 100 and rc == INVALID_ARG and 0 < m.max() and (m > 0).mean() > 0.5
    assert np.array_equal(match, m) and np.array_equal(filled, f)


# ---- 6. argument errors --------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(ctx):
    from circkit_amd import api
    recs = (b"ACGTTGCAAC" * 5, b"GATTACA" * 9)
    data, offs = S.pack(recs)
    b = Buffers(data, offs, 4)
    b.launch(ctx, 5)
    before = status(ctx)
    rows_before = b.result()
    lib, h = ctx._lib, ctx._h

    def call(p, d_bytes=b.d_bytes, d_offs=b.d_offs, d_rows=b.d_rows[GUARD:], d_counts=b.d_counts[GUARD:], by_ref=True):
        return lib.circkit_sketch_batch_device(h, api._ptr(d_bytes), api._ptr(d_offs), b.n, ctypes.byref(p) if by_ref else None, api._ptr(d_rows),
                                               api._ptr(d_counts))

    good = api.sketch_params(k=5, log2_bins=4)
    for kw in (dict(k=3), dict(k=33), dict(log2_bins=3), dict(log2_bins=11)):
        assert call(api.sketch_params(**{**dict(k=5, log2_bins=4), **kw})) == INVALID_ARG, kw
    for r in ((1, 0), (0, 1)):
        p = api.sketch_params(k=5, log2_bins=4)
        p.reserved[0], p.reserved[1] = r
        assert call(p) == INVALID_ARG
    assert call(good, by_ref=False) == INVALID_ARG
    assert call(good, d_bytes=None) == INVALID_ARG and call(good, d_offs=None) == INVALID_ARG and call(good, d_rows=None) == INVALID_ARG
    # the output over the offsets: the rows begin inside them, or the counts do
    off_as_rows = b.d_offs[1:]
    assert call(good, d_rows=off_as_rows) == INVALID_ARG and call(good, d_counts=b.d_offs.view(__import__("torch").int32)[1:]) == INVALID_ARG
    assert call(good, d_counts=b.d_rows[GUARD:].view(__import__("torch").int32)[2:]) == INVALID_ARG
    # the compare's
    d_pairs, d_res = _to(np.zeros((1, 2), dtype=np.int32)), _to(np.zeros((1, 2), dtype=np.int32))
    cmp = lambda a=b.d_rows[GUARD:], lb=4, pairs=d_pairs, res=d_res: lib.circkit_sketch_compare_device(  # noqa: E731
        h, api._ptr(a), 2, api._ptr(a), 2, lb, api._ptr(pairs), 1, api._ptr(res))
    assert cmp(lb=3) == INVALID_ARG and cmp(lb=11) == INVALID_ARG and cmp(a=None) == INVALID_ARG and cmp(pairs=None) == INVALID_ARG
    assert cmp(res=None) == INVALID_ARG and cmp(res=d_pairs) == INVALID_ARG
    assert lib.circkit_sketch_batch_device(None, None, None, 0, ctypes.byref(good), None, None) == INVALID_ARG
    # nothing ran: the status and every buffer are as they were
    assert status(ctx) == before
    after = b.result()
    assert np.array_equal(after[0], rows_before[0]) and np.array_equal(after[1], rows_before[1])
    assert call(good) == OK and status(ctx) == before


# ---- 7. one chain, the host forms, usefulness ------------------------------------------------------------------------------------
def test_text_to_sketch_to_compare(ctx):
    """FASTA text parsed on the device, sketched and compared without the batch leaving it, against the yardstick over the
    host-parsed records."""
    import circkit_amd
    import torch
    records, planted, unrelated = S.planted(5, n=12)
    text = b"".join(b">r%d some words\n" % i + b"\n".join(s[j:j + 70] for j in range(0, len(s), 70)).lower() + b"\n" for i, s in enumerate(records))
    _, h_data, h_offs, _ = circkit_amd.api.fasta_parse(text)
    host = tuple(bytes(h_data[int(h_offs[i]):int(h_offs[i + 1])]) for i in range(len(h_offs) - 1))
    assert host == records
    _, d_data, d_offs, _ = ctx.fasta_parse_text(text, keep_on_device=True)
    n = len(records)
    d_rows = torch.zeros(n * 256, dtype=torch.int64, device=_dev())
    d_counts = torch.zeros(n, dtype=torch.int32, device=_dev())
    pairs = np.array(planted + unrelated, dtype=np.uint32)
    d_pairs, d_res = _to(pairs.view(np.int32)), torch.zeros((len(pairs), 2), dtype=torch.int32, device=_dev())
    ctx.sketch_batch_device(d_data, d_offs, n, d_rows, d_counts, k=21, log2_bins=8)
    ctx.sketch_compare_device(d_rows, n, d_rows, n, 8, d_pairs, len(pairs), d_res)
    exp_rows, exp_counts = S.expected(host, 21, 8)
    assert ctx.sketch_status() == (int(exp_counts.sum()), 0) and ctx.sketch_compare_status() == 0
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64).reshape(n, 256), exp_rows)
    assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), exp_counts)
    m, f, _ = R.compare_pairs(exp_rows, exp_rows, pairs)
    res = d_res.cpu().numpy().view(np.uint32)
    assert np.array_equal(res[:, 0], m) and np.array_equal(res[:, 1], f)


def test_usefulness(ctx):
    """60 records, each planted once more with 1 % substitutions, a random rotation and a random strand: the device equals the
    yardstick exactly, and the yardstick scores every planted pair at 0.3 or more and every unrelated pair at 0.05 or less."""
    import circkit_amd
    records, planted, unrelated = S.planted(S.USEFUL_SEED)
    exp_rows, exp_counts = S.expected(records, 21, 8)
    rows, counts = circkit_amd.default_context().sketch_batch(*S.pack(records), k=21, log2_bins=8)
    assert np.array_equal(rows, exp_rows) and np.array_equal(counts, exp_counts)
    for pairs, holds in ((planted, lambda j: j.min() >= 0.3), (unrelated, lambda j: j.max() <= 0.05)):
        match, filled = circkit_amd.sketch_similarity(rows, rows, pairs)
        m, f, _ = R.compare_pairs(exp_rows, exp_rows, pairs)
        assert np.array_equal(match, m) and np.array_equal(filled, f)
        assert holds(m / f)


def test_host_forms(ctx):
    import circkit_amd
    from circkit_amd import api
    recs = S.length_records(16)[190:]
    rows, counts = circkit_amd.sketch_batch(recs, k=16, log2_bins=6, seed=9)
    exp = S.expected(recs, 16, 6, 9)
    assert rows.shape == (len(recs), 64) and rows.dtype == np.uint64 and np.array_equal(rows, exp[0]) and np.array_equal(counts, exp[1])
    rows0, counts0 = circkit_amd.sketch_batch([], k=16)
    assert rows0.shape == (0, 256) and len(counts0) == 0
    other = exp[0][:5].copy()
    pairs = [(0, 0), (len(recs) - 1, 4), (7, 2)]
    m, f = circkit_amd.sketch_similarity(rows, other, pairs)
    em, ef, _ = R.compare_pairs(exp[0], other, pairs)
    assert np.array_equal(m, em) and np.array_equal(f, ef)
    assert [len(x) for x in circkit_amd.sketch_similarity(rows, rows, [])] == [0, 0]
    with pytest.raises(circkit_amd.CirckitError) as e:
        circkit_amd.sketch_similarity(rows, other, [(0, 0), (0, 5)])
    assert e.value.code == INVALID_ARG
    # refused from the offsets alone: the payload is ten bytes
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    out, cnt = np.full((2, 16), 7, dtype=np.uint64), np.full(2, 7, dtype=np.uint32)
    p = api.sketch_params(k=4, log2_bins=4)
    for offs, code in (([0, 10, 10 + 2 ** 31], TOO_LONG), ([1, 10, 10], INVALID_ARG), ([0, 10, 4], INVALID_ARG)):
        offs = np.array(offs, dtype=np.uint64)
        assert ctx._lib.circkit_sketch_batch(ctx._h, api._ptr(data), api._ptr(offs), 2, ctypes.byref(p), api._ptr(out), api._ptr(cnt)) == code
    assert (out == 7).all() and (cnt == 7).all()
