"""GPU: circkit_windows_gather_device / _status / _of_records_device / circkit_orfs_windows_device / circkit_windows_gather
against the restatement tests/windows_ref.py: the case list of the CPU fiber test, capacities, refusals, the window lists of
rotate / cat / decat / revcomp, ORF sequences end to end, the chain reads -> ... -> ORFs -> ORF sequences, and the host forms.
Every byte and offset is compared; canaries surround the payload, the windows and both outputs."""
import os

import numpy as np
import pytest

from tests import windows_ref as R
from tests import windows_sets as S
from tests.orfs_ref import cyclic_cut

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY, OUT_CANARY, WIN_CANARY = 0x4E, 0x3F, 0x6B
OFF_CANARY = 0x25A5A5A5A5A5A5A5
OK, INVALID_ARG, OOM = 0, -1, -5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_examples")
_C = S.constants()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


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
    """(rc, total bytes, invalid windows) of the last gather, without raising."""
    import ctypes
    t, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_windows_status(ctx._h, ctypes.byref(t), ctypes.byref(bad))
    return rc, t.value, bad.value


class Buffers:
    """A batch and its windows on the device: the payload at in_shift mod 16 behind `lead` canary bytes (offsets[0] = lead), the
    output (`room` bytes) at out_shift mod 16, canaries round the payload, the windows and both outputs."""

    def __init__(self, data, offs, wins, room, in_shift=0, out_shift=0, lead=0):
        import torch
        self.n, self.m, self.room = len(offs) - 1, len(wins), room
        nb = len(data)
        raw = np.full(GUARD + in_shift + lead + nb + GUARD, IN_CANARY, dtype=np.uint8)
        raw[GUARD + in_shift + lead:GUARD + in_shift + lead + nb] = data
        self.raw_in = raw
        self.d_raw = _to(raw)
        self.d_bytes = self.d_raw[GUARD + in_shift:]
        self.offs = np.asarray(offs, dtype=np.uint64) + np.uint64(lead)
        self.d_offs = _to(_i64(self.offs))
        rw = np.full(GUARD + 24 * self.m + GUARD, WIN_CANARY, dtype=np.uint8)
        rw[GUARD:GUARD + 24 * self.m] = np.ascontiguousarray(wins, dtype=R.WINDOW_DTYPE).view(np.uint8)
        self.raw_win = rw
        self.d_raw_win = _to(rw)
        self.d_win = self.d_raw_win[GUARD:]
        self.d_raw_out = torch.full((GUARD + out_shift + room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        self.o0 = GUARD + out_shift
        self.d_out = self.d_raw_out[self.o0:]
        self.d_out_off = torch.full((GUARD + self.m + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
        assert self.d_bytes.data_ptr() % 16 == in_shift % 16 and self.d_out.data_ptr() % 16 == out_shift % 16 and self.d_win.data_ptr() % 8 == 0

    def launch(self, ctx, capacity=None):
        ctx.windows_gather_device(self.d_bytes, self.d_offs, self.n, self.d_win, self.m, self.d_out, self.room if capacity is None else capacity,
                                  self.d_out_off[GUARD:])

    def result(self, written):
        """(out bytes, out_offsets) after the canary checks; `written`: the bytes the gather may have written."""
        raw_out, off = self.d_raw_out.cpu().numpy(), _u64(self.d_out_off)
        assert np.array_equal(self.d_raw.cpu().numpy(), self.raw_in), "the gather wrote into its input"
        assert np.array_equal(_u64(self.d_offs), self.offs), "the gather wrote into the offsets"
        assert np.array_equal(self.d_raw_win.cpu().numpy(), self.raw_win), "the gather wrote into the windows"
        assert (raw_out[:self.o0] == OUT_CANARY).all() and (raw_out[self.o0 + written:] == OUT_CANARY).all(), "wrote outside [out, out + total)"
        assert (off[:GUARD] == OFF_CANARY).all() and (off[GUARD + self.m + 1:] == OFF_CANARY).all(), "out_offsets written outside its m + 1 entries"
        return raw_out[self.o0:self.o0 + written].copy(), off[GUARD:GUARD + self.m + 1].copy()


def check(ctx, data, offs, wins, what="", exp=None, **place):
    exp = exp if exp is not None else R.gather(data, offs, wins)
    b = Buffers(data, offs, wins, len(exp[0]), **place)
    b.launch(ctx)
    rc, total, bad = status(ctx)
    assert (total, bad) == (len(exp[0]), exp[2]) and rc == (INVALID_ARG if exp[2] else OK), (what, rc, total, bad)
    out, off = b.result(total)
    assert np.array_equal(off, exp[1]), what
    assert np.array_equal(out, exp[0]), what
    return exp


# ---- 1. the case list of the CPU fiber test ----------------------------------------------------------------------------------
CASES = S.all_cases(_C)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case_list(ctx, k):
    name, data, offs, wins, place = CASES[k]
    check(ctx, data, offs, wins, what=name, **place)


def test_case_list_covers_every_shift_and_a_lead():
    assert {c[4].get("in_shift", 0) for c in CASES} == set(range(16)) == {c[4].get("out_shift", 0) for c in CASES}
    assert any(c[4].get("lead", 0) for c in CASES)


def test_window_count_round_a_chunk_of_tile_sums(ctx):
    """One window more than a round of the scan's second level takes (WSCAN_WG tiles): one-byte windows, so that the expected
    bytes are one numpy expression; the first 3 000 and the last 3 000 are compared with the restatement as well."""
    rng = np.random.default_rng(12)
    data, offs = S.batch(rng)
    m = _C["WSCAN_CHUNK"] + 1
    w = np.zeros(m, dtype=R.WINDOW_DTYPE)
    w["length"] = 1
    w["record"] = rng.integers(1, len(S.RECORD_LENGTHS), size=m)
    w["start"] = rng.integers(0, 2 ** 32, size=m)
    n = np.diff(offs.astype(np.int64))[w["record"]]
    exp = data[offs.astype(np.int64)[w["record"]] + w["start"].astype(np.int64) % n]
    exp_off = np.arange(m + 1, dtype=np.uint64)
    for sl in (slice(0, 3000), slice(m - 3000, m)):
        assert np.array_equal(R.gather(data, offs, w[sl])[0], exp[sl])
    check(ctx, data, offs, w, what="chunk + 1", exp=(exp, exp_off, 0), out_shift=3)


# ---- 2. capacity -------------------------------------------------------------------------------------------------------------
def test_capacity(ctx):
    name, data, offs, wins, _ = S.shift_cases(np.random.default_rng(3))[5]
    wins = wins[:-2]                                                            # (no invalid windows: the status is the capacity's alone)
    exp, exp_off, _ = R.gather(data, offs, wins)
    total = len(exp)
    for capacity in (total, total - 1, 0):
        b = Buffers(data, offs, wins, total, in_shift=3, out_shift=11, lead=2)
        b.launch(ctx, capacity)
        rc, t, bad = status(ctx)
        assert (t, bad) == (total, 0)
        out, off = b.result(total if capacity == total else 0)                  # (beyond `written`, every byte must still be canary)
        assert np.array_equal(off, exp_off)
        if capacity == total:
            assert rc == OK and np.array_equal(out, exp)
        else:
            assert rc == OOM and str(total) in ctx._lib.circkit_last_error(ctx._h).decode()


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_null_pointers_and_rotation_by_zero(ctx):
    import circkit_amd
    import torch
    data, offs = S.batch(np.random.default_rng(4))
    wins = R.windows([(5, 4, 1, 0), (40, 9, 3, 1)])
    exp = R.gather(data, offs, wins)
    b = Buffers(data, offs, wins, len(exp[0]))
    args = dict(d_bytes=b.d_bytes, d_offsets=b.d_offs, n_records=b.n, d_windows=b.d_win, n_windows=b.m, d_out_bytes=b.d_out, out_capacity=b.room,
                d_out_offsets=b.d_out_off[GUARD:])
    for name in ("d_bytes", "d_offsets", "d_windows", "d_out_bytes", "d_out_offsets"):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.windows_gather_device(**dict(args, **{name: None}))
        assert e.value.code == INVALID_ARG and "null buffer" in str(e.value)
    assert ctx._lib.circkit_windows_gather_device(None, None, None, 0, None, 0, None, 0, None) == INVALID_ARG
    assert ctx._lib.circkit_windows_status(None, None, None) == INVALID_ARG
    check(ctx, data, offs, wins, what="after the refusals", exp=exp)
    d_win = torch.full((24 * b.n,), WIN_CANARY, dtype=torch.uint8, device=_dev())
    for kind, kw in (("rotate_bases", dict(bases=0)), ("rotate_percent", dict(percent=0.0)), ("rotate_percent", dict(percent=-0.0)), (5, dict()),
                     (2 ** 32 - 1, dict())):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.windows_of_records_device(b.d_offs, b.n, kind, d_win, **kw)
        assert e.value.code == INVALID_ARG and ("Rotation by 0 is not allowed" in str(e.value)) == isinstance(kind, str)
    for name in ("d_offsets", "d_windows"):
        with pytest.raises(circkit_amd.CirckitError):
            ctx.windows_of_records_device(**dict(dict(d_offsets=b.d_offs, n_records=b.n, kind="cat", d_windows=d_win), **{name: None}))
    with pytest.raises(circkit_amd.CirckitError):
        ctx.orfs_windows_device(None, d_win, b.n, 1, d_win)
    ctx.synchronize()
    assert (d_win.cpu().numpy() == WIN_CANARY).all(), "a refused call wrote windows"


def test_an_output_that_overlaps_the_payload(ctx):
    """The offsets are the device's, so the device refuses: nothing is written -- out_offsets aside, which is complete -- and the
    status carries the error.  An output that ends where the payload begins, or begins where it ends, does not overlap."""
    import torch
    data, offs = S.batch(np.random.default_rng(5))
    nb = len(data)
    wins = R.windows_of_records(np.diff(offs.astype(np.int64)), R.REVCOMP)
    exp, exp_off, _ = R.gather(data, offs, wins)
    assert len(exp) == nb
    whole = torch.full((GUARD + 3 * nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    whole[GUARD + nb:GUARD + 2 * nb] = _to(data)
    before = whole.cpu().numpy().copy()
    d_offs, d_win = _to(_i64(offs)), _to(wins.view(np.uint8))
    for out0, overlaps in ((GUARD, False), (GUARD + 1, True), (GUARD + nb, True), (GUARD + 2 * nb - 1, True), (GUARD + 2 * nb, False)):
        d_out_off = torch.full((len(wins) + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
        ctx.windows_gather_device(whole[GUARD + nb:], d_offs, len(offs) - 1, d_win, len(wins), whole[out0:], nb, d_out_off)
        rc, total, bad = status(ctx)
        off = _u64(d_out_off)
        assert (total, bad) == (nb, 0) and np.array_equal(off[:len(wins) + 1], exp_off) and (off[len(wins) + 1:] == OFF_CANARY).all()
        now = whole.cpu().numpy()
        if overlaps:
            assert rc == INVALID_ARG and "overlaps" in ctx._lib.circkit_last_error(ctx._h).decode()
            assert np.array_equal(now, before), "an overlapping output was written"
        else:
            assert rc == OK and np.array_equal(now[out0:out0 + nb], exp)
            now[out0:out0 + nb] = OUT_CANARY
            assert np.array_equal(now, before), "wrote outside [out, out + total), or into the payload"
            whole[out0:out0 + nb] = OUT_CANARY


def test_invalid_windows_are_counted_and_their_neighbours_written(ctx):
    data, offs = S.batch(np.random.default_rng(6))
    nr = len(offs) - 1
    bad = S.invalid_rows(nr)
    rows = []
    for k in range(40):
        rows += [(20 + k, 4 + k % 7, k, k & 1), bad[k % len(bad)]]
    exp = check(ctx, data, offs, R.windows(rows + [bad[0]] * 3), what="invalid windows", out_shift=5)
    assert exp[2] == 43 and len(exp[0]) == sum(20 + k for k in range(40))
    check(ctx, data, offs, R.windows(bad * 5), what="only invalid windows")
    # every window invalid because the batch has no record at all: nothing of the batch is dereferenced
    import torch
    wins = R.windows([(5, 0, 0, 0), (7, 1, 0, 1)])
    d_out_off = torch.full((3,), OFF_CANARY, dtype=torch.int64, device=_dev())
    ctx.windows_gather_device(None, None, 0, _to(wins.view(np.uint8)), 2, None, 0, d_out_off)
    assert status(ctx) == (INVALID_ARG, 0, 2) and _u64(d_out_off).tolist() == [0, 0, 0]


def test_no_windows(ctx):
    import torch
    data, offs = S.batch(np.random.default_rng(7))
    d_out_off = torch.full((4,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_out = torch.full((64,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.windows_gather_device(_to(data), _to(_i64(offs)), len(offs) - 1, None, 0, d_out, 64, d_out_off)
    assert status(ctx) == (OK, 0, 0)
    assert _u64(d_out_off).tolist() == [0, OFF_CANARY, OFF_CANARY, OFF_CANARY] and (d_out.cpu().numpy() == OUT_CANARY).all()
    ctx.windows_gather_device(None, None, 0, None, 0, None, 0, None)
    assert status(ctx) == (OK, 0, 0)


# ---- 4. one window per record ------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 999, 1000, 1001, 2_000_003]
PERCENTS = (0.5, 0.25, 0.999, 1.0, 1.5, -0.5, 1e30, -1e30, float("nan"))


def rotate_grid():
    bases = sorted({b for n in (3, 1000, 2_000_003) for b in (1, -1, 3, -3, n, n + 1, -(n + 1), 2 ** 63 - 1, -2 ** 63)})
    return [("rotate_bases", R.ROTATE_BASES, dict(bases=b)) for b in bases] + [("rotate_percent", R.ROTATE_PERCENT, dict(percent=p)) for p in PERCENTS]


def test_windows_of_records(ctx):
    import torch
    offs = np.zeros(len(LENGTHS) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(LENGTHS)
    d_offs = _to(_i64(offs + np.uint64(11)))                                    # offsets[0] != 0
    n = len(LENGTHS)
    for name, kind, kw in rotate_grid() + [("cat", R.CAT, {}), ("decat", R.DECAT, {}), ("revcomp", R.REVCOMP, {})]:
        d_win = torch.full((GUARD + 24 * n + GUARD,), WIN_CANARY, dtype=torch.uint8, device=_dev())
        ctx.windows_of_records_device(d_offs, n, name, d_win[GUARD:], **kw)
        ctx.synchronize()
        got = d_win.cpu().numpy()
        assert (got[:GUARD] == WIN_CANARY).all() and (got[GUARD + 24 * n:] == WIN_CANARY).all()
        exp = R.windows_of_records(LENGTHS, kind, **kw)
        assert np.array_equal(got[GUARD:GUARD + 24 * n].view(R.WINDOW_DTYPE), exp), (name, kw)


def test_rotated_long_record_among_short_ones(ctx):
    rng = np.random.default_rng(8)
    data, offs = S.batch(rng, LENGTHS)
    lengths = np.diff(offs.astype(np.int64))
    for kind, kw in ((R.ROTATE_PERCENT, dict(percent=0.37)), (R.ROTATE_BASES, dict(bases=-(2_000_003 + 1))), (R.REVCOMP, {}), (R.CAT, {})):
        wins = R.windows_of_records(lengths, kind, **kw)
        check(ctx, data, offs, wins, what=(kind, kw), in_shift=5, out_shift=9, lead=3)


def fixture_batch(name):
    from oracle import oracle as O
    text = open(os.path.join(GOLDEN, name, "in.fasta"), "rb").read()
    return (text,) + S.pack_like(O.full_seq(raw) for _, raw in O.read_fasta(text))


@pytest.mark.parametrize("name", ("rotate_5", "rotate_minus_5", "rotate_0.25", "rotate_0.5", "cat", "decat"))
def test_rotate_cat_decat_on_the_fixtures(ctx, name):
    """Windows on the device, then the gather, against the sequences oracle.cli_rotate / cli_cat / cli_decat write."""
    from oracle import oracle as O
    from tests.test_windows_cpu import expected_rotate, rotate_bases, written_sequences
    text, data, offs = fixture_batch(name)
    n = len(offs) - 1
    lengths = np.diff(offs.astype(np.int64))
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    import torch
    d_win = torch.zeros(24 * n, dtype=torch.uint8, device=_dev())
    d_out = torch.zeros(2 * len(data), dtype=torch.uint8, device=_dev())
    d_out_off = torch.zeros(n + 1, dtype=torch.int64, device=_dev())

    def on_device(kind, **kw):
        ctx.windows_of_records_device(d_offs, n, kind, d_win, **kw)
        ctx.windows_gather_device(d_bytes, d_offs, n, d_win, n, d_out, len(d_out), d_out_off)
        total, bad = ctx.windows_status()
        assert bad == 0
        return S.split(d_out.cpu().numpy()[:total], _u64(d_out_off))
    assert on_device("cat") == written_sequences(O.cli_cat(text))
    assert on_device("decat") == written_sequences(O.cli_decat(text))
    for b in sorted({b for x in set(lengths.tolist()) for b in rotate_bases(x)}):
        assert on_device("rotate_bases", bases=b) == expected_rotate(text, bases=b), b
    for p in PERCENTS:
        assert on_device("rotate_percent", percent=p) == expected_rotate(text, percent=p), p


def test_revcomp_batch_per_record(ctx):
    import circkit_amd
    from oracle import oracle as O
    data, offs = S.batch(np.random.default_rng(9), S.RECORD_LENGTHS + [4097, 0, 5])
    for form in (ctx.revcomp_batch, circkit_amd.revcomp_batch):
        out, out_off = form(data, offs)
        assert np.array_equal(out_off, offs)
        raw = bytes(data)
        assert S.split(out, out_off) == [O.revcomp(raw[int(a):int(b)]) for a, b in zip(offs[:-1], offs[1:])]


# ---- 5. ORF sequences end to end ---------------------------------------------------------------------------------------------
def orf_set():
    """20 000 ACGT records of 200 b .. 3 kb and the adversarial records of tests/windows_sets.orf_records."""
    rng = np.random.default_rng(61)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lens = np.exp(rng.uniform(np.log(200), np.log(3000), size=20000)).astype(np.int64)
    body = acgt[rng.integers(0, 4, size=int(lens.sum()))]
    extra = S.orf_records(count=0)
    data = np.concatenate([body, np.frombuffer(b"".join(extra), dtype=np.uint8)])
    offs = np.zeros(len(lens) + len(extra) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.concatenate([lens, [len(s) for s in extra]]))
    return data, offs


@pytest.fixture(scope="module")
def orf_batch():
    """(data, offsets, device payload, device offsets, the records' bytes, their reverse complements): computed once, unchanged."""
    from oracle import oracle as O
    data, offs = orf_set()
    raw = bytes(data)
    recs = [raw[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    return data, offs, _to(data), _to(_i64(offs)), recs, [O.revcomp(r) for r in recs]


def expected_sequences(recs, rcs, orf_off, orfs, include_stop):
    cut = 0 if include_stop else 3
    rec = np.repeat(np.arange(len(orf_off) - 1), np.diff(orf_off.astype(np.int64))).tolist()
    return [cyclic_cut((rcs if st else recs)[r], s, L - cut)
            for r, s, L, st in zip(rec, orfs["start"].tolist(), orfs["length"].tolist(), orfs["strand"].tolist())]


def device_orf_sequences(ctx, d_bytes, d_offs, n, cap, room, include_stop, **kw):
    """orfs_batch_device -> orfs_status -> orfs_windows_device -> windows_gather_device: (orf offsets, ORFs, sequences)."""
    import circkit_amd
    import torch
    d_orf_off = torch.zeros(n + 1, dtype=torch.int64, device=_dev())
    d_orfs = torch.zeros(cap * 24, dtype=torch.uint8, device=_dev())
    ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, cap, **kw)
    total = ctx.orfs_status()
    d_win = torch.zeros(max(total, 1) * 24, dtype=torch.uint8, device=_dev())
    d_seq_off = torch.full((total + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_seq = torch.full((room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.orfs_windows_device(d_orf_off, d_orfs, n, total, d_win, include_stop=include_stop)
    ctx.windows_gather_device(d_bytes, d_offs, n, d_win, total, d_seq, room, d_seq_off)
    B, bad = ctx.windows_status()
    assert bad == 0
    seq_off = _u64(d_seq_off)
    assert (seq_off[total + 1:] == OFF_CANARY).all() and int(seq_off[total]) == B and (d_seq[B:].cpu().numpy() == OUT_CANARY).all()
    return _u64(d_orf_off), d_orfs.cpu().numpy().view(circkit_amd.api.ORF_DTYPE)[:total], S.split(d_seq[:B].cpu().numpy(), seq_off[:total + 1])


@pytest.mark.parametrize("strands", (1, 2, 3))
@pytest.mark.parametrize("mode", (0, 1))
def test_orf_sequences_on_the_device(ctx, orf_batch, mode, strands):
    from tests import orfs_ref
    data, offs, d_bytes, d_offs, recs, rcs = orf_batch
    n = len(offs) - 1
    kw = dict(min_length=75, require_stop=True, strands=strands, mode=mode)
    eo, e = orfs_ref.orfs_batch(data, offs, threads=16, **kw)
    assert len(e) > n // 2
    for include_stop in (False, True):
        orf_off, orfs, seqs = device_orf_sequences(ctx, d_bytes, d_offs, n, len(e), int(e["length"].sum()), include_stop, **kw)
        assert np.array_equal(orf_off, eo) and np.array_equal(orfs, e)
        assert seqs == expected_sequences(recs, rcs, eo, e, include_stop), (mode, strands, include_stop)


@pytest.mark.parametrize("include_stop", (False, True))
def test_orf_sequences_are_the_lines_circkit_orfs_writes_on_every_record(ctx, orf_batch, include_stop):
    """Mode 0, both strands, the CLI's default flags, all 20 000 generated records and the adversarial ones: the sequences in
    order are the sequence lines of orfs_ref.cli_orfs."""
    from tests import orfs_ref
    data, offs, d_bytes, d_offs, recs, _ = orf_batch
    want = S.sequence_lines(orfs_ref.cli_orfs(S.fasta_of(recs), include_stop=include_stop)[0])
    _, _, got = device_orf_sequences(ctx, d_bytes, d_offs, len(recs), len(want), sum(len(w) for w in want), include_stop,
                                     min_length=75, require_stop=True, strands=3, mode=0)
    assert len(want) > len(recs) and got == want


def test_orf_sequences_are_the_lines_circkit_orfs_writes(ctx, orf_batch):
    """Mode 0, both strands, the CLI's default flags and `--no-stop-required` with three start codons (multi-lap ORFs on the
    records without a stop), through the device chain and both host forms: the concatenation is the sequence lines of
    orfs_ref.cli_orfs.  The first 2 000 generated records and the adversarial ones (the test above has every record under the
    default flags): four runs of cli_orfs and eight host-form round trips in one test."""
    import circkit_amd
    from tests import orfs_ref
    data, offs, _, _, recs, _ = orf_batch
    seqs = recs[:2000] + recs[20000:]
    sub, sub_offs = S.pack_like(seqs)
    d_bytes, d_offs = _to(sub), _to(_i64(sub_offs))
    fasta = S.fasta_of(seqs)
    for flags, kw in ((dict(), dict(min_length=75, require_stop=True)),
                      (dict(no_stop_required=True, start_codons="ATG,CTG,TTG"), dict(min_length=75, require_stop=False, start_codons=["ATG", "CTG", "TTG"]))):
        for include_stop in (False, True):
            want = S.sequence_lines(orfs_ref.cli_orfs(fasta, include_stop=include_stop, **flags)[0])
            _, orfs, got = device_orf_sequences(ctx, d_bytes, d_offs, len(seqs), len(sub), 8 * len(sub), include_stop, strands=3, mode=0, **kw)
            assert got == want and len(want) > 1000
            if flags:
                assert (orfs["wraps"] > 0).any() and (orfs["stop"] == circkit_amd.api.ORF_NO_STOP).any()
            for form in (ctx.orf_sequences, circkit_amd.orf_sequences):
                h_off, h_orfs, h_seq, h_seq_off = form(sub, sub_offs, include_stop=include_stop, strands=3, mode=0, **kw)
                assert np.array_equal(h_orfs, orfs) and S.split(h_seq, h_seq_off) == want


# ---- 6. the chain reads -> monomers -> canonical forms -> unique records -> ORFs -> ORF sequences ------------------------------
def test_chain_reads_to_orf_sequences(ctx):
    """The chain of tests/test_uniq_compact_gpu.py::test_chain_reads_to_orfs, continued: nothing but the status calls' totals comes
    home before the final compare, and two gathers with different window lists run back to back, their statuses read after both."""
    import torch
    from oracle import oracle as O
    from tests import mono_ref, mono_sets, monomers_ref, orfs_ref, uniq_compact_ref
    n = 2000
    data, offs = mono_sets.rolling(33, [1000] * n)
    data = data.copy().reshape(n, 1000)
    rng = np.random.default_rng(34)
    for i in range(4, n, 4):
        data[i] = data[int(rng.integers(0, i))]
    data = data.reshape(-1)
    params = dict(seed_len=10, min_identity=0.95)
    # the CPU side
    ends = mono_ref.batch(data, offs, threads=16, **params)
    mono, moff, msrc, _ = monomers_ref.compact(data, offs, ends)
    canon, hashes = O.canonicalize_batch(mono, moff, True, True, threads=16)
    u = uniq_compact_ref.compact(canon, moff, O.uniq_first_seen(hashes))
    eo, e = orfs_ref.orfs_batch(u[0], u[1], threads=16)
    assert len(e) > 100
    exp_cut = R.gather(u[0], u[1], R.orf_windows(eo, e, False))
    exp_all = R.gather(u[0], u[1], R.orf_windows(eo, e, True))
    assert len(exp_all[0]) == len(exp_cut[0]) + 3 * len(e)
    # the device side
    dev = _dev()
    nb = len(data)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_end = torch.empty(n, dtype=torch.int32, device=dev)
    d_mono = torch.empty(nb, dtype=torch.uint8, device=dev)
    d_moff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_msrc = torch.empty(n, dtype=torch.int64, device=dev)
    ctx.monomerize_batch_device(d_bytes, d_offs, n, d_end, **params)
    ctx.monomers_compact_device(d_bytes, d_offs, n, d_end, d_mono, d_moff, d_msrc)
    m, B = ctx.monomers_status()
    d_canon = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)
    d_hash = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    d_fs = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    d_uniq = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)
    d_uoff = torch.empty(m + 1, dtype=torch.int64, device=dev)
    d_usrc = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    ctx.canonicalize_batch_device(d_mono, d_moff, m, out_bytes=d_canon, out_xxh3=d_hash)
    ctx.uniq_resolve_device(d_hash, m, 0, d_fs)
    ctx.uniq_compact_device(d_canon, d_moff, m, d_fs, d_uniq, d_uoff, d_usrc)
    ctx.uniq_status()
    m2, B2 = ctx.uniq_compact_status()
    cap = 2 * B2 + 16
    d_orf_off = torch.zeros(m2 + 1, dtype=torch.int64, device=dev)
    d_orfs = torch.zeros(cap * 24, dtype=torch.uint8, device=dev)
    ctx.orfs_batch_device(d_uniq, d_uoff, m2, d_orf_off, d_orfs, cap)
    total = ctx.orfs_status()
    assert total == len(e)
    room = len(exp_all[0])
    outs = []
    for include_stop in (False, True):                                         # back to back: no status, no copy between the two
        d_win = torch.empty(total * 24, dtype=torch.uint8, device=dev)
        d_seq = torch.full((room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=dev)
        d_seq_off = torch.empty(total + 1, dtype=torch.int64, device=dev)
        ctx.orfs_windows_device(d_orf_off, d_orfs, m2, total, d_win, include_stop=include_stop)
        ctx.windows_gather_device(d_uniq, d_uoff, m2, d_win, total, d_seq, room, d_seq_off)
        outs.append((d_seq, d_seq_off))
    assert ctx.windows_status() == (len(exp_all[0]), 0)                         # the second gather's
    for (d_seq, d_seq_off), exp in zip(outs, (exp_cut, exp_all)):
        got = d_seq.cpu().numpy()
        assert np.array_equal(_u64(d_seq_off), exp[1])
        assert np.array_equal(got[:len(exp[0])], exp[0]) and (got[len(exp[0]):] == OUT_CANARY).all()


# ---- 7. the host forms -------------------------------------------------------------------------------------------------------
def test_host_gather_reports_the_total_and_succeeds_on_the_retry(ctx):
    import ctypes
    name, data, offs, wins, _ = S.shift_cases(np.random.default_rng(3))[0]
    wins = wins[:-2]
    exp, exp_off, _ = R.gather(data, offs, wins)
    total = ctypes.c_uint64(0)
    out = np.full(len(exp) + GUARD, OUT_CANARY, dtype=np.uint8)
    out_off = np.full(len(wins) + 1, OFF_CANARY, dtype=np.uint64)
    call = lambda cap: ctx._lib.circkit_windows_gather(ctx._h, data.ctypes.data, offs.ctypes.data, len(offs) - 1, wins.ctypes.data, len(wins),
                                                       out.ctypes.data, cap, out_off.ctypes.data, ctypes.byref(total))
    assert call(len(exp) - 1) == OOM and total.value == len(exp) and np.array_equal(out_off, exp_off) and (out == OUT_CANARY).all()
    assert status(ctx) == (OOM, len(exp), 0)
    assert call(len(exp)) == OK and np.array_equal(out[:len(exp)], exp) and (out[len(exp):] == OUT_CANARY).all()
    assert status(ctx) == (OK, len(exp), 0)
    got, got_off = ctx.windows_gather(data, offs, np.concatenate([wins] * 40))   # more than the payload: grows and runs again
    assert np.array_equal(got, np.tile(exp, 40)) and int(got_off[-1]) == 40 * len(exp)


def test_host_forms_round_trip(ctx):
    import circkit_amd
    data, offs = S.batch(np.random.default_rng(10), [0, 1, 2, 7, 100, 1000, 33])
    out, out_off = ctx.cat_batch(data, offs)
    assert np.array_equal(out_off, 2 * offs)
    back, back_off = circkit_amd.decat_batch(out, out_off)
    assert np.array_equal(back, data) and np.array_equal(back_off, offs)
    for kw in (dict(bases=5), dict(percent=0.37), dict(bases=-2 ** 63)):
        there, t_off = ctx.rotate_batch(data, offs, **kw)
        assert np.array_equal(t_off, offs) and not np.array_equal(there, data)
        exp = R.gather(data, offs, R.windows_of_records(np.diff(offs.astype(np.int64)), R.ROTATE_PERCENT if "percent" in kw else R.ROTATE_BASES, **kw))
        assert np.array_equal(there, exp[0])
    there, _ = circkit_amd.rotate_batch(data, offs, bases=5)
    back, _ = circkit_amd.rotate_batch(there, offs, bases=-5)
    assert np.array_equal(back, data)
    twice, _ = ctx.revcomp_batch(*ctx.revcomp_batch(data, offs))
    assert np.array_equal(twice, data)                                          # (the table is an involution)
    with pytest.raises(circkit_amd.CirckitError):
        ctx.rotate_batch(data, offs, bases=0)
    with pytest.raises(ValueError):
        ctx.rotate_batch(data, offs)
    # records but not one payload byte, and no records at all: empty records back, not an error
    for e_offs in (np.zeros(3, dtype=np.uint64), np.zeros(1, dtype=np.uint64)):
        nothing = np.zeros(0, dtype=np.uint8)
        for got in (ctx.cat_batch(nothing, e_offs), ctx.decat_batch(nothing, e_offs), ctx.revcomp_batch(nothing, e_offs),
                    ctx.rotate_batch(nothing, e_offs, bases=3), ctx.rotate_batch(nothing, e_offs, percent=0.5)):
            assert len(got[0]) == 0 and np.array_equal(got[1], e_offs)
    w = np.zeros(2, dtype=R.WINDOW_DTYPE)
    w["length"], w["record"], w["strand"] = [5, 1], [0, 1], [0, 1]
    out, out_off = ctx.windows_gather(np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64), w)
    assert len(out) == 0 and np.array_equal(out_off, np.zeros(3, dtype=np.uint64))
