"""GPU: circkit_windows_translate_device / circkit_translate_status / circkit_windows_translate against the restatement
tests/translate_ref.py: the case list of the CPU fiber test, window counts round the scan's tiles, capacities, refusals, invalid
windows, a gather and a translate on one ctx, ORF proteins end to end, the chain reads -> ... -> ORFs -> proteins, and the host
forms.  Every residue and offset is compared; canaries surround the payload, the windows and both outputs."""
import ctypes

import numpy as np
import pytest

from tests import test_windows_gpu as G
from tests import translate_ref as T
from tests import translate_sets as TS
from tests import windows_ref as R
from tests import windows_sets as S
from tests.orfs_ref import cyclic_cut

pytestmark = pytest.mark.gpu

GUARD, OUT_CANARY, OFF_CANARY = G.GUARD, G.OUT_CANARY, G.OFF_CANARY
OK, INVALID_ARG, OOM = 0, -1, -5
_C = TS.constants()
_dev, _to, _i64, _u64 = G._dev, G._to, G._i64, G._u64


@pytest.fixture(scope="module")
def ctx():
    """A ctx that launches on torch's current stream, so that the tensors torch fills and the ctx's kernels are ordered."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def params(code):
    from circkit_amd import api
    aa, unknown, first_as_m = code
    return api.translate_params(table=aa, unknown=unknown, first_as_m=first_as_m)


def status(ctx):
    """(rc, total residues, invalid windows) of the last translate, without raising."""
    t, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_translate_status(ctx._h, ctypes.byref(t), ctypes.byref(bad))
    return rc, t.value, bad.value


class Buffers(G.Buffers):
    """The gather test's device buffers (canaries round the payload, the windows and both outputs), launched as a translate."""

    def launch(self, ctx, code, capacity=None):
        ctx.windows_translate_device(self.d_bytes, self.d_offs, self.n, self.d_win, self.m, self.d_out, self.room if capacity is None else capacity,
                                     self.d_out_off[GUARD:], params=params(code))


def check(ctx, data, offs, wins, code, what="", exp=None, **place):
    exp = exp if exp is not None else T.windows_translate(data, offs, wins, *code)
    b = Buffers(data, offs, wins, len(exp[0]), **place)
    b.launch(ctx, code)
    rc, total, bad = status(ctx)
    assert (total, bad) == (len(exp[0]), exp[2]) and rc == (INVALID_ARG if exp[2] else OK), (what, rc, total, bad)
    out, off = b.result(total)
    assert np.array_equal(off, exp[1]), what
    assert np.array_equal(out, exp[0]), what
    return exp


# ---- 1. the case list of the CPU fiber test ----------------------------------------------------------------------------------
CASES = TS.all_cases(_C)


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case_list(ctx, k):
    name, data, offs, wins, place, code = CASES[k]
    check(ctx, data, offs, wins, code, what=name, **place)


def test_case_list_covers_the_scan_tile(ctx):
    counts = {len(c[3]) for c in CASES}
    assert _C["WSCAN_TILE"] == 2048 and {2047, 2048, 2049} <= counts


def test_window_count_round_a_chunk_of_tile_sums(ctx):
    """One window more than a round of the scan's second level takes (WSCAN_WG tiles): windows of one codon on strand 0, so that
    the expected residues are one numpy expression; the first 3 000 and the last 3 000 are compared with the restatement too."""
    rng = np.random.default_rng(12)
    data, offs = TS.batch(rng)
    code = TS.CODES[2]
    m = _C["WSCAN_CHUNK"] + 1
    w = np.zeros(m, dtype=R.WINDOW_DTYPE)
    w["length"] = rng.integers(3, 6, size=m)                                    # one residue each
    w["record"] = rng.integers(1, len(TS.RECORD_LENGTHS), size=m)
    w["start"] = rng.integers(0, 2 ** 32, size=m)
    n = np.diff(offs.astype(np.int64))[w["record"]]
    r0 = offs.astype(np.int64)[w["record"]]
    codons = np.stack([data[r0 + (w["start"].astype(np.int64) + k) % n] for k in range(3)], axis=1).reshape(-1)
    exp, exp_off = T.translate_packed(codons, 3 * np.arange(m + 1, dtype=np.uint64), *code)
    assert np.array_equal(exp_off, np.arange(m + 1, dtype=np.uint64))
    for sl in (slice(0, 3000), slice(m - 3000, m)):
        assert np.array_equal(T.windows_translate(data, offs, w[sl], *code)[0], exp[sl])
    check(ctx, data, offs, w, code, what="chunk + 1", exp=(exp, exp_off, 0), out_shift=3)


# ---- 2. capacity and the refusals ----------------------------------------------------------------------------------------------
def test_capacity(ctx):
    name, data, offs, wins, _, code = TS.shift_cases(np.random.default_rng(3))[5]
    wins = wins[:-2]                                                            # (no invalid windows: the status is the capacity's alone)
    exp, exp_off, _ = T.windows_translate(data, offs, wins, *code)
    total = len(exp)
    for capacity in (total, total - 1, 0):
        b = Buffers(data, offs, wins, total, in_shift=3, out_shift=11, lead=2)
        b.launch(ctx, code, capacity)
        rc, t, bad = status(ctx)
        assert (t, bad) == (total, 0)
        out, off = b.result(total if capacity == total else 0)                  # (beyond `written`, every byte must still be canary)
        assert np.array_equal(off, exp_off)
        if capacity == total:
            assert rc == OK and np.array_equal(out, exp)
        else:
            assert rc == OOM and str(total) in ctx._lib.circkit_last_error(ctx._h).decode()


def test_refused_before_anything_is_enqueued(ctx):
    """Null pointers, first_as_m beyond 1 and reserved bytes in use: INVALID_ARG, the outputs still canary, and the status still
    the previous translate's."""
    import circkit_amd
    from circkit_amd import api
    data, offs = TS.batch(np.random.default_rng(4))
    code = TS.CODES[0]
    wins = R.windows([(15, 6, 1, 0), (120, 13, 3, 1)])
    exp = check(ctx, data, offs, wins, code, what="before the refusals")
    b = Buffers(data, offs, wins, len(exp[0]))
    args = dict(d_bytes=b.d_bytes, d_offsets=b.d_offs, n_records=b.n, d_windows=b.d_win, n_windows=b.m, d_out_aa=b.d_out, out_capacity=b.room,
                d_out_offsets=b.d_out_off[GUARD:], params=params(code))
    for name in ("d_bytes", "d_offsets", "d_windows", "d_out_aa", "d_out_offsets"):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.windows_translate_device(**dict(args, **{name: None}))
        assert e.value.code == INVALID_ARG and "null buffer" in str(e.value)
    raw = (b.d_bytes.data_ptr(), b.d_offs.data_ptr(), b.n, b.d_win.data_ptr(), b.m)
    tail = (b.d_out.data_ptr(), b.room, b.d_out_off[GUARD:].data_ptr())
    assert ctx._lib.circkit_windows_translate_device(ctx._h, *raw, None, *tail) == INVALID_ARG
    bad_params = [api.translate_params(), api.translate_params()] + [api.translate_params() for _ in range(6)]
    bad_params[0].first_as_m, bad_params[1].first_as_m = 2, 255
    for k in range(6):
        bad_params[2 + k].reserved[k] = 1 + k
    for p in bad_params:
        assert ctx._lib.circkit_windows_translate_device(ctx._h, *raw, ctypes.byref(p), *tail) == INVALID_ARG
        out_off = np.zeros(b.m + 1, dtype=np.uint64)
        assert ctx._lib.circkit_windows_translate(ctx._h, data.ctypes.data, offs.ctypes.data, b.n, wins.ctypes.data, b.m, ctypes.byref(p), None, 0,
                                                  out_off.ctypes.data, None) == INVALID_ARG
    assert ctx._lib.circkit_windows_translate_device(None, None, None, 0, None, 0, None, None, 0, None) == INVALID_ARG
    assert ctx._lib.circkit_translate_status(None, None, None) == INVALID_ARG
    assert status(ctx) == (OK, len(exp[0]), 0)
    got = b.d_raw_out.cpu().numpy()
    assert (got == OUT_CANARY).all() and (_u64(b.d_out_off) == OFF_CANARY).all(), "a refused call wrote"


def test_an_output_that_overlaps_the_payload(ctx):
    """The offsets are the device's, so the device refuses: nothing is written -- out_offsets aside, which is complete -- and the
    status carries the error.  An output that ends where the payload begins, or begins where it ends, does not overlap."""
    import torch
    data, offs = TS.batch(np.random.default_rng(5))
    nb = len(data)
    code = TS.CODES[3]
    wins = R.windows_of_records(np.diff(offs.astype(np.int64)), R.CAT)[::-1].copy()
    exp, exp_off, _ = T.windows_translate(data, offs, wins, *code)
    na = len(exp)
    assert nb // 2 < na < nb
    whole = torch.full((GUARD + 3 * nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    whole[GUARD + nb:GUARD + 2 * nb] = _to(data)
    before = whole.cpu().numpy().copy()
    d_offs, d_win = _to(_i64(offs)), _to(wins.view(np.uint8))
    for out0, overlaps in ((GUARD + nb - na, False), (GUARD + nb - na + 1, True), (GUARD + nb, True), (GUARD + 2 * nb - 1, True), (GUARD + 2 * nb, False)):
        d_out_off = torch.full((len(wins) + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
        ctx.windows_translate_device(whole[GUARD + nb:], d_offs, len(offs) - 1, d_win, len(wins), whole[out0:], nb, d_out_off, params=params(code))
        rc, total, bad = status(ctx)
        off = _u64(d_out_off)
        assert (total, bad) == (na, 0) and np.array_equal(off[:len(wins) + 1], exp_off) and (off[len(wins) + 1:] == OFF_CANARY).all()
        now = whole.cpu().numpy()
        if overlaps:
            assert rc == INVALID_ARG and "overlaps" in ctx._lib.circkit_last_error(ctx._h).decode()
            assert np.array_equal(now, before), "an overlapping output was written"
        else:
            assert rc == OK and np.array_equal(now[out0:out0 + na], exp)
            now[out0:out0 + na] = OUT_CANARY
            assert np.array_equal(now, before), "wrote outside [out, out + total), or into the payload"
            whole[out0:out0 + na] = OUT_CANARY


def test_invalid_windows_are_counted_and_their_neighbours_written(ctx):
    data, offs = TS.batch(np.random.default_rng(6))
    nr = len(offs) - 1
    bad = S.invalid_rows(nr)
    rows = []
    for k in range(40):
        rows += [(60 + k, 6 + k % 9, k, k & 1), bad[k % len(bad)]]
    exp = check(ctx, data, offs, R.windows(rows + [bad[0]] * 3), TS.CODES[1], what="invalid windows", out_shift=5)
    assert exp[2] == 43 and len(exp[0]) == sum((60 + k) // 3 for k in range(40))
    check(ctx, data, offs, R.windows(bad * 5), TS.CODES[0], what="only invalid windows")
    # every window invalid because the batch has no record at all: nothing of the batch is dereferenced
    import torch
    wins = R.windows([(5, 0, 0, 0), (7, 1, 0, 1)])
    d_out_off = torch.full((3,), OFF_CANARY, dtype=torch.int64, device=_dev())
    ctx.windows_translate_device(None, None, 0, _to(wins.view(np.uint8)), 2, None, 0, d_out_off)
    assert status(ctx) == (INVALID_ARG, 0, 2) and _u64(d_out_off).tolist() == [0, 0, 0]


def test_no_windows_and_records_without_a_payload_byte(ctx):
    import torch
    data, offs = TS.batch(np.random.default_rng(7))
    d_out_off = torch.full((4,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_out = torch.full((64,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.windows_translate_device(_to(data), _to(_i64(offs)), len(offs) - 1, None, 0, d_out, 64, d_out_off)
    assert status(ctx) == (OK, 0, 0)
    assert _u64(d_out_off).tolist() == [0, OFF_CANARY, OFF_CANARY, OFF_CANARY] and (d_out.cpu().numpy() == OUT_CANARY).all()
    ctx.windows_translate_device(None, None, 0, None, 0, None, 0, None)
    assert status(ctx) == (OK, 0, 0)
    wins = R.windows([(9, 0, 0, 0), (30, 2, 5, 1), (3, 1, 0, 0)])                # three empty records, one byte of memory that nobody reads
    d_one = torch.full((1,), G.IN_CANARY, dtype=torch.uint8, device=_dev())
    ctx.windows_translate_device(d_one, _to(_i64(np.zeros(4, dtype=np.uint64))), 3, _to(wins.view(np.uint8)), 3, d_out, 64, d_out_off)
    assert status(ctx) == (OK, 0, 0)
    assert _u64(d_out_off).tolist() == [0, 0, 0, 0] and (d_out.cpu().numpy() == OUT_CANARY).all()


# ---- 3. a gather and a translate on one ctx ------------------------------------------------------------------------------------
def test_each_status_reports_its_own_totals(ctx):
    data, offs = TS.batch(np.random.default_rng(8))
    code = TS.CODES[2]
    wins = R.windows([(100, 13, 7, 1), (31, 6, 2, 0), (1000, 14, 999, 0)])
    wins_bad = R.windows([(40, 12, 0, 0), (5, 99, 0, 0)])
    exp_g, exp_t = R.gather(data, offs, wins), T.windows_translate(data, offs, wins_bad, *code)
    g = G.Buffers(data, offs, wins, len(exp_g[0]))
    t = Buffers(data, offs, wins_bad, len(exp_t[0]))
    g.launch(ctx)
    t.launch(ctx, code)
    assert status(ctx) == (INVALID_ARG, 13, 1) and G.status(ctx) == (OK, 1131, 0)
    t2 = Buffers(data, offs, wins, 376, out_shift=1)                             # 33 + 10 + 333 residues
    t2.launch(ctx, code, capacity=375)
    g2 = G.Buffers(data, offs, wins_bad, 40)
    g2.launch(ctx)
    assert G.status(ctx) == (INVALID_ARG, 40, 1) and status(ctx) == (OOM, 376, 0) and G.status(ctx) == (INVALID_ARG, 40, 1)
    assert np.array_equal(g.result(1131)[0], exp_g[0]) and np.array_equal(t.result(13)[0], exp_t[0])
    assert np.array_equal(g2.result(40)[0], R.gather(data, offs, wins_bad)[0]) and len(t2.result(0)[0]) == 0


def test_two_translates_back_to_back(ctx):
    """No status and no copy between the two: each writes its own outputs, the status is the second one's."""
    data, offs = TS.batch(np.random.default_rng(9))
    wins_a = R.windows(TS.grid(TS.RECORD_LENGTHS[6:], lambda n: [n, 3 * n + 1], lambda n: [n - 2]))
    wins_b = wins_a[::-1][:17].copy()
    exp_a, exp_b = T.windows_translate(data, offs, wins_a, *TS.CODES[1]), T.windows_translate(data, offs, wins_b, *TS.CODES[2])
    a = Buffers(data, offs, wins_a, len(exp_a[0]), out_shift=7)
    b = Buffers(data, offs, wins_b, len(exp_b[0]), in_shift=2)
    a.launch(ctx, TS.CODES[1])
    b.launch(ctx, TS.CODES[2])
    assert status(ctx) == (OK, len(exp_b[0]), 0)
    for buf, exp in ((a, exp_a), (b, exp_b)):
        out, off = buf.result(len(exp[0]))
        assert np.array_equal(off, exp[1]) and np.array_equal(out, exp[0])


# ---- 4. ORF proteins end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def orf_batch():
    """(data, offsets, device payload, device offsets, the records' bytes, their reverse complements): computed once, unchanged."""
    from oracle import oracle as O
    data, offs = G.orf_set()
    raw = bytes(data)
    recs = [raw[int(a):int(b)] for a, b in zip(offs[:-1], offs[1:])]
    return data, offs, _to(data), _to(_i64(offs)), recs, [O.revcomp(r) for r in recs]


def device_orfs(ctx, d_bytes, d_offs, n, cap, **kw):
    import circkit_amd
    import torch
    d_orf_off = torch.zeros(n + 1, dtype=torch.int64, device=_dev())
    d_orfs = torch.zeros(cap * 24, dtype=torch.uint8, device=_dev())
    ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, cap, **kw)
    total = ctx.orfs_status()
    return d_orf_off, d_orfs, total, _u64(d_orf_off), d_orfs.cpu().numpy().view(circkit_amd.api.ORF_DTYPE)[:total].copy()


def device_proteins(ctx, d_bytes, d_offs, n, d_orf_off, d_orfs, total, room, include_stop, code):
    """orfs_windows_device -> windows_translate_device on an ORF batch the device holds: (residues, offsets)."""
    import torch
    d_win = torch.zeros(max(total, 1) * 24, dtype=torch.uint8, device=_dev())
    d_aa_off = torch.full((total + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_aa = torch.full((room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.orfs_windows_device(d_orf_off, d_orfs, n, total, d_win, include_stop=include_stop)
    ctx.windows_translate_device(d_bytes, d_offs, n, d_win, total, d_aa, room, d_aa_off, params=params(code))
    B, bad = ctx.translate_status()
    assert bad == 0
    aa_off = _u64(d_aa_off)
    assert (aa_off[total + 1:] == OFF_CANARY).all() and int(aa_off[total]) == B and (d_aa[B:].cpu().numpy() == OUT_CANARY).all()
    return d_aa[:B].cpu().numpy(), aa_off[:total + 1]


def code_of(table, first_as_m):
    return (T.genetic_codes()[table], b"X", first_as_m)


@pytest.mark.parametrize("strands", (1, 2, 3))
@pytest.mark.parametrize("mode", (0, 1))
def test_orf_proteins_on_the_device(ctx, orf_batch, mode, strands):
    """Every protein against translate(cyclic_cut(...)) of the ORF the device reports (tests/test_orfs_gpu*.py hold the ORF
    lists to the restatement): without the stop under table 1, with it under table 4 and first_as_m."""
    data, offs, d_bytes, d_offs, recs, rcs = orf_batch
    n = len(offs) - 1
    kw = dict(min_length=75, require_stop=True, strands=strands, mode=mode)
    d_orf_off, d_orfs, total, orf_off, orfs = device_orfs(ctx, d_bytes, d_offs, n, 16 * n, **kw)
    # the generator's conditions
    assert total > (n if strands == 3 else n // 2) and (orfs["wraps"] >= 1).any()
    assert set(np.unique(orfs["strand"]).tolist()) == {1: {0}, 2: {1}, 3: {0, 1}}[strands]
    with_stop = G.expected_sequences(recs, rcs, orf_off, orfs, True)
    for include_stop, code in ((False, code_of(1, False)), (True, code_of(4, True))):
        seqs, seq_offs = S.pack_like(with_stop if include_stop else [s[:-3] for s in with_stop])
        exp, exp_off = T.translate_packed(seqs, seq_offs, *code)
        got, got_off = device_proteins(ctx, d_bytes, d_offs, n, d_orf_off, d_orfs, total, len(exp), include_stop, code)
        assert np.array_equal(got_off, exp_off) and np.array_equal(got, exp), (mode, strands, include_stop)
        if include_stop:
            last = got[exp_off[1:].astype(np.int64) - 1]
            assert set(np.unique(last).tolist()) <= {ord("*"), ord("W")} and (last == ord("W")).any() and (got[exp_off[:-1].astype(np.int64)] == ord("M")).all()


def test_orf_proteins_are_the_translated_lines_circkit_orfs_writes(ctx, orf_batch):
    """Mode 0, both strands, the CLI's default flags and `--no-stop-required` with three start codons, with and without the
    stop, through the device chain and both host forms: the proteins in order are translate() of the sequence lines of
    orfs_ref.cli_orfs.  The first 2 000 generated records and the adversarial ones: the Python writer is the slow part."""
    import circkit_amd
    from tests import orfs_ref
    data, offs, _, _, recs, _ = orf_batch
    seqs = recs[:2000] + recs[20000:]
    sub, sub_offs = S.pack_like(seqs)
    n = len(seqs)
    d_bytes, d_offs = _to(sub), _to(_i64(sub_offs))
    fasta = S.fasta_of(seqs)
    for flags, kw in ((dict(), dict(min_length=75, require_stop=True)),
                      (dict(no_stop_required=True, start_codons="ATG,CTG,TTG"), dict(min_length=75, require_stop=False, start_codons=["ATG", "CTG", "TTG"]))):
        d_orf_off, d_orfs, total, _, orfs = device_orfs(ctx, d_bytes, d_offs, n, len(sub), strands=3, mode=0, **kw)
        assert bool(flags) == bool((orfs["stop"] == circkit_amd.api.ORF_NO_STOP).any()) and (orfs["wraps"] >= 1).any()
        for include_stop in (False, True):
            lines = S.sequence_lines(orfs_ref.cli_orfs(fasta, include_stop=include_stop, **flags)[0])
            table, first_as_m = (4, True) if flags else (1, False)
            code = code_of(table, first_as_m)
            exp, exp_off = T.translate_packed(*S.pack_like(lines), *code)
            assert len(lines) > 1000 and (exp == ord("X")).any()
            got, got_off = device_proteins(ctx, d_bytes, d_offs, n, d_orf_off, d_orfs, total, len(exp) + 5, include_stop, code)
            assert np.array_equal(got_off, exp_off) and np.array_equal(got, exp), (flags, include_stop)
            for form in (ctx.orf_proteins, circkit_amd.orf_proteins):
                h_off, h_orfs, h_aa, h_aa_off = form(sub, sub_offs, include_stop=include_stop, table=table, first_as_m=first_as_m, strands=3, mode=0, **kw)
                assert np.array_equal(h_orfs, orfs) and np.array_equal(h_aa, exp) and np.array_equal(h_aa_off, exp_off)


# ---- 5. the chain reads -> monomers -> canonical forms -> unique records -> ORFs -> proteins ----------------------------------
def test_chain_reads_to_proteins(ctx):
    """The chain of tests/test_windows_gpu.py::test_chain_reads_to_orf_sequences with the translate in the gather's place: nothing
    but the status calls' totals comes home before the final compare."""
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
    mparams = dict(seed_len=10, min_identity=0.95)
    code = code_of(11, False)
    # the CPU side
    ends = mono_ref.batch(data, offs, threads=16, **mparams)
    mono, moff, msrc, _ = monomers_ref.compact(data, offs, ends)
    canon, hashes = O.canonicalize_batch(mono, moff, True, True, threads=16)
    u = uniq_compact_ref.compact(canon, moff, O.uniq_first_seen(hashes))
    eo, e = orfs_ref.orfs_batch(u[0], u[1], threads=16)
    assert len(e) > 100
    exp = [T.translate_packed(*R.gather(u[0], u[1], R.orf_windows(eo, e, stop))[:2], *code) for stop in (False, True)]
    assert len(exp[1][0]) == len(exp[0][0]) + len(e)
    # the device side
    dev = _dev()
    nb = len(data)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_end = torch.empty(n, dtype=torch.int32, device=dev)
    d_mono = torch.empty(nb, dtype=torch.uint8, device=dev)
    d_moff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_msrc = torch.empty(n, dtype=torch.int64, device=dev)
    ctx.monomerize_batch_device(d_bytes, d_offs, n, d_end, **mparams)
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
    room = len(exp[1][0])
    outs = []
    for include_stop in (False, True):                                         # back to back: no status, no copy between the two
        d_win = torch.empty(total * 24, dtype=torch.uint8, device=dev)
        d_aa = torch.full((room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=dev)
        d_aa_off = torch.empty(total + 1, dtype=torch.int64, device=dev)
        ctx.orfs_windows_device(d_orf_off, d_orfs, m2, total, d_win, include_stop=include_stop)
        ctx.windows_translate_device(d_uniq, d_uoff, m2, d_win, total, d_aa, room, d_aa_off, params=params(code))
        outs.append((d_aa, d_aa_off))
    assert ctx.translate_status() == (room, 0)                                  # the second translate's
    for (d_aa, d_aa_off), (want, want_off) in zip(outs, exp):
        got = d_aa.cpu().numpy()
        assert np.array_equal(_u64(d_aa_off), want_off)
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == OUT_CANARY).all()


# ---- 6. the host forms -------------------------------------------------------------------------------------------------------
def test_host_translate_reports_the_total_and_succeeds_on_the_retry(ctx):
    import circkit_amd
    name, data, offs, wins, _, code = TS.shift_cases(np.random.default_rng(3))[0]
    wins = wins[:-2]
    exp, exp_off, _ = T.windows_translate(data, offs, wins, *code)
    p = params(code)
    total = ctypes.c_uint64(0)
    out = np.full(len(exp) + GUARD, OUT_CANARY, dtype=np.uint8)
    out_off = np.full(len(wins) + 1, OFF_CANARY, dtype=np.uint64)
    call = lambda cap: ctx._lib.circkit_windows_translate(ctx._h, data.ctypes.data, offs.ctypes.data, len(offs) - 1, wins.ctypes.data, len(wins),
                                                          ctypes.byref(p), out.ctypes.data, cap, out_off.ctypes.data, ctypes.byref(total))
    assert call(len(exp) - 1) == OOM and total.value == len(exp) and np.array_equal(out_off, exp_off) and (out == OUT_CANARY).all()
    assert status(ctx) == (OOM, len(exp), 0)
    assert call(len(exp)) == OK and np.array_equal(out[:len(exp)], exp) and (out[len(exp):] == OUT_CANARY).all()
    assert status(ctx) == (OK, len(exp), 0)
    many = np.concatenate([wins] * 40)                                          # more than the first buffer holds: grows and runs again
    assert 40 * len(exp) > max(len(data) // 3, 1)
    for got, got_off in (ctx.windows_translate(data, offs, many, params=p), ctx.windows_translate(data, offs, many, capacity=1, params=p),
                         circkit_amd.windows_translate(data, offs, many, table=code[0], unknown=code[1], first_as_m=code[2])):
        assert np.array_equal(got, np.tile(exp, 40)) and int(got_off[-1]) == 40 * len(exp)
    with pytest.raises(circkit_amd.CirckitError):
        ctx.windows_translate(data, offs, R.windows([(9, 99, 0, 0)]))
    w = R.windows([(9, 0, 0, 0), (3, 1, 0, 1)])
    out, out_off = ctx.windows_translate(np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64), w)
    assert len(out) == 0 and np.array_equal(out_off, np.zeros(3, dtype=np.uint64))
    h = ctx.orf_proteins(np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.uint64))
    assert len(h[1]) == 0 and len(h[2]) == 0 and h[3].tolist() == [0]
