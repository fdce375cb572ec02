"""GPU: circkit_uniq_compact_device / _status / circkit_uniq_batch against the restatement tests/uniq_compact_ref.py, behind
every uniq path of the ABI (crafted first_seen, resolve, streaming insert + lookup), and the chain reads -> monomers ->
canonical forms -> unique records -> ORFs against the CPU side.  Every byte and index is compared; canaries surround all five
outputs and the input."""
import os

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S
from tests import monomers_ref as MR
from tests import monomers_sets as MS
from tests import uniq_compact_ref as UR
from tests.test_monomers_compact_cpu import SCAN_COUNTS

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
OFF_CANARY, SRC_CANARY = 0x25A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A
DSRC_CANARY, DFIRST_CANARY = 0x1C1C1C1C1C1C1C1C, 0x2D2D2D2D2D2D2D2D
BIG_BASE = 2 ** 40 + 7
NOT_FOUND = UR.NOT_FOUND

# Both sides of a scan tile and of a chunk of CSCAN_WG tile sums, from the kernel's constants; 0, 1, 2 and two tiles + 1
_C = MS.constants()
TILE, CHUNK, TILE_BYTES = _C["CSCAN_TILE"], _C["CSCAN_CHUNK"], _C["TILE_BYTES"]
COUNTS = [0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1]
assert {TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1} <= set(SCAN_COUNTS)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _u64(t, k=None):
    a = t.cpu().numpy().view(np.uint64)
    return a if k is None else a[:k]


@pytest.fixture(scope="module")
def ctx():
    """A ctx that launches on torch's current stream, so that the tensors torch fills and the ctx's kernels are ordered."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


class Buffers:
    """A batch on the device: the payload at in_shift mod 16 behind `lead` canary bytes (offsets[0] = lead), the output at
    out_shift mod 16, canaries round the payload and all five outputs."""

    def __init__(self, data, offs, first_seen, in_shift=0, out_shift=0, lead=0):
        import torch
        self.n = n = len(offs) - 1
        self.nb = nb = len(data)
        raw = np.full(GUARD + in_shift + lead + nb + GUARD, IN_CANARY, dtype=np.uint8)
        raw[GUARD + in_shift + lead:GUARD + in_shift + lead + nb] = data
        self.raw_in = raw
        self.d_raw = _to(raw)
        self.d_bytes = self.d_raw[GUARD + in_shift:]
        self.d_offs = _to(_i64(np.asarray(offs, dtype=np.uint64) + np.uint64(lead)))
        self.fs = np.ascontiguousarray(first_seen, dtype=np.uint64)
        self.d_fs = _to(_i64(self.fs)) if n else torch.zeros(1, dtype=torch.int64, device=_dev())
        self.d_raw_out = torch.full((GUARD + out_shift + nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        self.o0 = GUARD + out_shift
        self.d_out = self.d_raw_out[self.o0:]
        full = lambda k, v: torch.full((GUARD + k + GUARD,), v, dtype=torch.int64, device=_dev())
        self.d_out_off, self.d_out_src = full(n + 1, OFF_CANARY), full(n, SRC_CANARY)
        self.d_dup_src, self.d_dup_first = full(n, DSRC_CANARY), full(n, DFIRST_CANARY)
        assert self.d_bytes.data_ptr() % 16 == in_shift % 16 and self.d_out.data_ptr() % 16 == out_shift % 16

    def launch(self, ctx, base=0, dup_src=True, dup_first=True):
        ctx.uniq_compact_device(self.d_bytes, self.d_offs, self.n, self.d_fs, self.d_out, self.d_out_off[GUARD:], self.d_out_src[GUARD:],
                                base_index=base, d_dup_src=self.d_dup_src[GUARD:] if dup_src else None,
                                d_dup_first=self.d_dup_first[GUARD:] if dup_first else None)

    def result(self, m, B, dup_src=True, dup_first=True):
        """(out_data, out_offsets, out_src, dup_src | None, dup_first | None) after the canary checks."""
        n = self.n
        raw_out = self.d_raw_out.cpu().numpy()
        out_off, out_src = _u64(self.d_out_off), _u64(self.d_out_src)
        dsrc, dfirst = _u64(self.d_dup_src), _u64(self.d_dup_first)
        assert np.array_equal(self.d_raw.cpu().numpy(), self.raw_in), "the compact wrote into its input"
        if n:
            assert np.array_equal(_u64(self.d_fs), self.fs), "the compact wrote into first_seen"
        assert 0 <= m <= n and 0 <= B <= self.nb
        assert (raw_out[:self.o0] == OUT_CANARY).all() and (raw_out[self.o0 + B:] == OUT_CANARY).all(), "wrote outside [out, out + B)"
        assert (out_off[:GUARD] == OFF_CANARY).all() and (out_off[GUARD + m + 1:] == OFF_CANARY).all(), "out_offsets written beyond entry m"
        assert (out_src[:GUARD] == SRC_CANARY).all() and (out_src[GUARD + m:] == SRC_CANARY).all(), "out_src written beyond entry m - 1"
        for name, a, canary, want in (("dup_src", dsrc, DSRC_CANARY, dup_src), ("dup_first", dfirst, DFIRST_CANARY, dup_first)):
            if want:
                assert (a[:GUARD] == canary).all() and (a[GUARD + n - m:] == canary).all(), "%s written beyond entry n - m - 1" % name
            else:
                assert (a == canary).all(), "%s written though not asked for" % name
        assert int(out_off[GUARD + m]) == B
        return (raw_out[self.o0:self.o0 + B].copy(), out_off[GUARD:GUARD + m + 1].copy(), out_src[GUARD:GUARD + m].copy(),
                dsrc[GUARD:GUARD + n - m].copy() if dup_src else None, dfirst[GUARD:GUARD + n - m].copy() if dup_first else None)


def check(ctx, data, offs, fs, base=0, dup_src=True, dup_first=True, what="", exp=None, **place):
    exp = exp if exp is not None else UR.compact(data, offs, fs, base)
    b = Buffers(data, offs, fs, **place)
    b.launch(ctx, base, dup_src, dup_first)
    m, B = ctx.uniq_compact_status()
    assert (m, B) == (len(exp[2]), len(exp[0])), (what, m, B)
    UR.assert_equal(b.result(m, B, dup_src, dup_first), exp, (what, base, dup_src, dup_first, place))
    return exp


def crafted(rng, n, p_keep, base):
    """first_seen for n records: kept with probability p_keep, else an earlier index of this batch, an index of an earlier
    batch (base > 0) or ~0."""
    i = np.arange(n, dtype=np.uint64)
    own = np.uint64(base) + i
    earlier = np.uint64(base) + (rng.random(n) * i).astype(np.uint64)                      # < base + i for i >= 1
    before = rng.integers(0, base, size=n, dtype=np.uint64) if base else np.full(n, NOT_FOUND, dtype=np.uint64)
    kind = rng.integers(0, 3, size=n)
    drop = np.where(kind == 0, earlier, np.where(kind == 1, before, np.uint64(NOT_FOUND)))
    drop = np.where(drop == own, np.uint64(NOT_FOUND), drop).astype(np.uint64)             # (record 0 has no earlier one)
    keep = rng.random(n) < p_keep
    return np.where(keep, own, drop).astype(np.uint64)


DUP_FORMS = ((True, True), (False, True), (True, False), (False, False))


# ---- crafted first_seen: no hashing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
def test_crafted_first_seen(ctx, count):
    """Record counts on both sides of a scan tile and of a chunk of tile sums, records of 0..40 bytes, keep probability 0, 0.5
    and 1, both bases, dropped values of all three kinds, with and without each dup pointer.  The small counts run every
    combination; the large ones every (probability, base) pair with the four dup forms dealt round, all four at 0.5."""
    rng = np.random.default_rng(count)
    data, offs = MS.batch(rng, rng.integers(0, 41, size=count))
    k = 0
    for p in (0.5, 0.0, 1.0):
        for base in (0, BIG_BASE):
            fs = crafted(rng, count, p, base)
            exp = UR.compact(data, offs, fs, base)
            assert len(exp[2]) == (count if p == 1.0 else 0 if p == 0.0 else len(exp[2]))
            forms = DUP_FORMS if count <= 2 * TILE + 1 else (DUP_FORMS[k % 4], DUP_FORMS[(k + 2) % 4]) if p == 0.5 else (DUP_FORMS[k % 4],)
            for ds, df in forms:
                check(ctx, data, offs, fs, base, ds, df, what="crafted %d p=%g" % (count, p), exp=exp, out_shift=(count + k) % 16,
                      in_shift=(3 * k) % 16, lead=k)
            k += 1


# ---- the gather's tile edges -----------------------------------------------------------------------------------------------
def test_kept_bytes_round_a_gather_tile(ctx):
    rng = np.random.default_rng(5)
    for B in (TILE_BYTES - 1, TILE_BYTES, TILE_BYTES + 1):
        lengths = [17, B - 73, 5, 3, 0, 0, 70, 9]
        keep = [False, True, False, True, True, False, True, False]
        data, offs = MS.batch(rng, lengths)
        fs = np.where(keep, np.arange(8, dtype=np.uint64), np.array([NOT_FOUND, 0, 1, 0, 0, 4, 0, 6], dtype=np.uint64))
        exp = check(ctx, data, offs, fs, what="kept bytes %d" % B)
        assert len(exp[0]) == B and exp[2].tolist() == [1, 3, 4, 6]


def test_record_boundary_on_the_tile_boundary_at_every_output_shift(ctx):
    rng = np.random.default_rng(6)
    for a in (0, 1, 8, 15):
        first = TILE_BYTES - a                                                  # its end is the absolute end of the first tile
        lengths = [40, first, 3, 11, 0, 70]
        data, offs = MS.batch(rng, lengths)
        fs = np.array([NOT_FOUND, 1, 2, 1, 4, 5], dtype=np.uint64)
        exp = check(ctx, data, offs, fs, what="tile end", out_shift=a, in_shift=(a + 5) % 16, lead=11)
        assert exp[1].tolist() == [0, first, first + 3, first + 3, first + 73]


# ---- degenerate batches ----------------------------------------------------------------------------------------------------
def test_all_kept_and_all_dropped(ctx):
    rng = np.random.default_rng(7)
    n = 3000
    data, offs = MS.batch(rng, rng.integers(0, 41, size=n))
    for base in (0, BIG_BASE):
        own = np.uint64(base) + np.arange(n, dtype=np.uint64)
        exp = check(ctx, data, offs, own, base, what="all kept", out_shift=5)
        assert np.array_equal(exp[0], data) and np.array_equal(exp[2], np.arange(n)) and len(exp[3]) == 0
        fs = np.where(np.arange(n) % 2 == 0, np.uint64(NOT_FOUND), own + np.uint64(1)).astype(np.uint64)
        exp = check(ctx, data, offs, fs, base, what="all dropped", in_shift=3)
        assert len(exp[0]) == 0 and exp[1].tolist() == [0] and np.array_equal(exp[3], np.arange(n)) and np.array_equal(exp[4], fs)


def test_zero_length_records_kept_and_dropped(ctx):
    rng = np.random.default_rng(8)
    lengths = [3, 0, 0, 0, 5, 0, 1, 0, 0] * 30 + [0] * 70 + [2] + [0] * 70
    n = len(lengths)
    data, offs = MS.batch(rng, lengths)
    fs = np.where(np.arange(n) % 3 == 1, 0, np.arange(n)).astype(np.uint64)
    exp = check(ctx, data, offs, fs, what="empty records", out_shift=9, lead=3)
    assert (np.diff(exp[1].astype(np.int64)) == 0).sum() > 50 and (np.asarray(lengths)[exp[3].astype(np.int64)] == 0).sum() > 50
    data, offs = MS.batch(rng, [0] * 100)                                      # records, but no payload at all
    exp = check(ctx, data, offs, np.where(np.arange(100) % 2 == 0, np.arange(100), 0).astype(np.uint64), what="only empty records")
    assert len(exp[2]) == 50 and len(exp[0]) == 0


def test_one_3_mb_record_among_short_ones(ctx):
    rng = np.random.default_rng(9)
    lengths = [5, 0, 31, 3_000_000, 7, 1, 40, 0, 12]
    data, offs = MS.batch(rng, lengths)
    for fs in ([0, 1, 0, 3, 4, NOT_FOUND, 6, 7, 2], [0, 1, 0, 2, 4, NOT_FOUND, 6, 7, 2]):         # the long one kept, then dropped
        for place in (dict(), dict(in_shift=5, out_shift=11, lead=3)):
            exp = check(ctx, data, offs, np.array(fs, dtype=np.uint64), what="3 MB", **place)
            assert (len(exp[0]) > 3_000_000) == (fs[3] == 3)


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable(ctx):
    """Every refused call returns before it touches memory: the null checks on the host, the overlap check in the scan's
    single-workgroup kernel, ahead of the apply and the gather."""
    import circkit_amd
    import torch
    rng = np.random.default_rng(41)
    data, offs = MS.batch(rng, [40, 100, 7, 0, 22])
    fs = np.array([0, 0, 2, 3, NOT_FOUND], dtype=np.uint64)
    b = Buffers(data, offs, fs)
    args = dict(d_bytes=b.d_bytes, d_offsets=b.d_offs, n_records=b.n, d_first_seen=b.d_fs, d_out_bytes=b.d_out, d_out_offsets=b.d_out_off[GUARD:],
                d_out_src=b.d_out_src[GUARD:])
    for name in ("d_bytes", "d_offsets", "d_first_seen", "d_out_bytes", "d_out_offsets", "d_out_src"):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.uniq_compact_device(**dict(args, **{name: None}))
        assert e.value.code == -1 and "null buffer" in str(e.value), str(e.value)
        check(ctx, data, offs, fs, what="after a refusal")                      # the next valid call works
    assert ctx._lib.circkit_uniq_compact_device(None, None, None, 0, None, 0, *([None] * 5)) == -1
    assert ctx._lib.circkit_uniq_compact_status(None, None, None) == -1
    # An output whose owed room (as many bytes as the payload) overlaps the input payload: the offsets are the device's, so
    # the device refuses.  Nothing is written -- out_offsets[0] aside --, the totals are 0 and the status carries the error.
    # An output that ends where the payload begins, or begins where it ends, does not overlap.
    nb = b.nb
    whole = torch.full((GUARD + 3 * nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    whole[GUARD + nb:GUARD + 2 * nb] = _to(data)
    before = whole.cpu().numpy().copy()
    d_offs = _to(_i64(offs))
    exp = UR.compact(data, offs, fs)
    for out0, overlaps in ((GUARD, False), (GUARD + 1, True), (GUARD + nb, True), (GUARD + 2 * nb - 1, True), (GUARD + 2 * nb, False)):
        side = Buffers(data, offs, fs)                                          # fresh index outputs, canaries all over
        ctx.uniq_compact_device(whole[GUARD + nb:], d_offs, b.n, b.d_fs, whole[out0:], side.d_out_off[GUARD:], side.d_out_src[GUARD:],
                                d_dup_src=side.d_dup_src[GUARD:], d_dup_first=side.d_dup_first[GUARD:])
        if overlaps:
            with pytest.raises(circkit_amd.CirckitError) as e:
                ctx.uniq_compact_status()
            assert e.value.code == -1 and "overlaps" in str(e.value)
            assert np.array_equal(whole.cpu().numpy(), before), "an overlapping output was written"
            off = _u64(side.d_out_off)
            assert int(off[GUARD]) == 0 and (np.delete(off, GUARD) == OFF_CANARY).all()
            assert (_u64(side.d_out_src) == SRC_CANARY).all() and (_u64(side.d_dup_src) == DSRC_CANARY).all()
            assert (_u64(side.d_dup_first) == DFIRST_CANARY).all()
            check(ctx, data, offs, fs, what="after an overlap")
        else:
            m, B = ctx.uniq_compact_status()
            assert (m, B) == (len(exp[2]), len(exp[0]))
            now = whole.cpu().numpy()
            assert np.array_equal(now[out0:out0 + B], exp[0])
            now[out0:out0 + B] = OUT_CANARY
            assert np.array_equal(now, before), "wrote outside [out, out + B), or into the payload"
            whole[out0:out0 + B] = OUT_CANARY
            assert np.array_equal(_u64(side.d_dup_src)[GUARD:GUARD + b.n - m], exp[3])


def test_empty_batches(ctx):
    import torch
    d_out_off = torch.full((4,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_one = torch.zeros(1, dtype=torch.int64, device=_dev())
    ctx.uniq_compact_device(None, d_one, 0, None, None, d_out_off, None)
    assert ctx.uniq_compact_status() == (0, 0)
    assert d_out_off.cpu().numpy().tolist() == [0, OFF_CANARY, OFF_CANARY, OFF_CANARY]
    ctx.uniq_compact_device(None, None, 0, None, None, None, None)
    assert ctx.uniq_compact_status() == (0, 0)


# ---- independence ------------------------------------------------------------------------------------------------------------
def test_monomer_and_uniq_compacts_keep_their_own_totals(ctx):
    import torch
    rng = np.random.default_rng(51)
    lengths = rng.integers(0, 41, size=500)
    data, offs = MS.batch(rng, lengths)
    ends = np.where(rng.random(500) < 0.7, lengths // 2, MR.NONE).astype(np.uint32)
    mexp = MR.compact(data, offs, ends)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_mono = torch.zeros(len(data), dtype=torch.uint8, device=_dev())
    d_moff = torch.zeros(501, dtype=torch.int64, device=_dev())
    d_msrc = torch.zeros(500, dtype=torch.int64, device=_dev())
    ctx.monomers_compact_device(d_bytes, d_offs, 500, _to(ends.view(np.int32)), d_mono, d_moff, d_msrc)
    fs = crafted(rng, 500, 0.3, 0)
    uexp = UR.compact(data, offs, fs)
    b = Buffers(data, offs, fs, out_shift=2)
    b.launch(ctx)
    mono, uniq = (len(mexp[2]), len(mexp[0])), (len(uexp[2]), len(uexp[0]))
    assert mono != uniq and mono[0] and uniq[0]
    assert ctx.monomers_status() == mono and ctx.uniq_compact_status() == uniq
    assert ctx.monomers_status() == mono                                        # and again, after the other status call
    UR.assert_equal(b.result(*uniq), uexp, "uniq compact behind a monomer compact")
    assert np.array_equal(d_mono.cpu().numpy()[:mono[1]], mexp[0]) and np.array_equal(_u64(d_msrc, mono[0]), mexp[2])
    # the other way round: a monomer compact behind the uniq compact does not disturb the uniq totals
    ctx.monomers_compact_device(d_bytes, d_offs, 500, _to(ends.view(np.int32)), d_mono, d_moff, d_msrc, keep_all=True)
    kexp = MR.compact(data, offs, ends, keep_all=True)
    assert ctx.uniq_compact_status() == uniq and ctx.monomers_status() == (500, len(kexp[0])) != mono


def test_back_to_back_compacts_on_one_stream(ctx):
    """Two uniq compacts with no synchronisation between them: the status reports the second, both outputs are right."""
    rng = np.random.default_rng(31)
    n = 5000
    data, offs = MS.batch(rng, rng.integers(0, 41, size=n), b"ACGT")
    fa, fb = crafted(rng, n, 0.8, 0), crafted(rng, n, 0.3, BIG_BASE)
    a, b = Buffers(data, offs, fa, out_shift=4), Buffers(data, offs, fb, in_shift=9)
    a.launch(ctx, 0)
    b.launch(ctx, BIG_BASE)
    ea, eb = UR.compact(data, offs, fa, 0), UR.compact(data, offs, fb, BIG_BASE)
    assert ctx.uniq_compact_status() == (len(eb[2]), len(eb[0]))
    assert (len(ea[2]), len(ea[0])) != (len(eb[2]), len(eb[0]))
    UR.assert_equal(a.result(len(ea[2]), len(ea[0])), ea, "first of two")
    UR.assert_equal(b.result(len(eb[2]), len(eb[0])), eb, "second of two")


# ---- the resolve path ------------------------------------------------------------------------------------------------------
def planted_set(seed=61, n=20000):
    """n ACGT records of 200 b .. 3 kb; every third is a rotation or the reverse complement of an earlier one."""
    rng = np.random.default_rng(seed)
    lengths = np.exp(rng.uniform(np.log(200), np.log(3000), size=n)).astype(np.int64)
    codes = []
    for i in range(n):
        if i % 3 == 2:
            src = codes[int(rng.integers(0, i))]
            k = int(rng.integers(0, len(src)))
            c = np.concatenate([src[k:], src[:k]]) if rng.random() < 0.5 else (3 - src[::-1])
        else:
            c = rng.integers(0, 4, size=int(lengths[i]), dtype=np.uint8)
        codes.append(c)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(c) for c in codes])
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate(codes)], offs


@pytest.fixture(scope="module")
def planted():
    """(data, offsets, canonical bytes, hashes, first_seen) of the planted set, computed once on the CPU and left unchanged."""
    from oracle import oracle as O
    data, offs = planted_set()
    canon, hashes = O.canonicalize_batch(data, offs, True, True, threads=16)
    fs = O.uniq_first_seen(hashes)
    kept = int(UR.keep_mask(fs).sum())
    assert 0.6 * len(fs) < kept < 0.7 * len(fs)
    return data, offs, canon, hashes, fs


def test_resolve_then_compact(ctx, planted):
    import torch
    data, offs, canon, hashes, fs = planted
    n, nb = len(offs) - 1, len(data)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_canon = torch.zeros(nb, dtype=torch.uint8, device=_dev())
    d_hash = torch.zeros(n, dtype=torch.int64, device=_dev())
    d_fs = torch.zeros(n, dtype=torch.int64, device=_dev())
    ctx.canonicalize_batch_device(d_bytes, d_offs, n, out_bytes=d_canon, out_xxh3=d_hash)
    ctx.uniq_resolve_device(d_hash, n, 0, d_fs)
    for name, d_payload, payload in (("canonical", d_canon, canon), ("input", d_bytes, data)):
        d_out = torch.full((nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        d_out_off = torch.full((n + 1,), OFF_CANARY, dtype=torch.int64, device=_dev())
        d_out_src = torch.full((n,), SRC_CANARY, dtype=torch.int64, device=_dev())
        d_dsrc = torch.full((n,), DSRC_CANARY, dtype=torch.int64, device=_dev())
        d_dfirst = torch.full((n,), DFIRST_CANARY, dtype=torch.int64, device=_dev())
        ctx.uniq_compact_device(d_payload, d_offs, n, d_fs, d_out, d_out_off, d_out_src, d_dup_src=d_dsrc, d_dup_first=d_dfirst)
        ctx.uniq_status()
        m, B = ctx.uniq_compact_status()
        exp = UR.compact(payload, offs, fs)
        assert (m, B) == (len(exp[2]), len(exp[0])), name
        out = d_out.cpu().numpy()
        UR.assert_equal((out[:B], _u64(d_out_off, m + 1), _u64(d_out_src, m), _u64(d_dsrc, n - m), _u64(d_dfirst, n - m)), exp, name)
        assert (out[B:] == OUT_CANARY).all() and (_u64(d_out_off)[m + 1:] == OFF_CANARY).all() and (_u64(d_out_src)[m:] == SRC_CANARY).all()
        assert (_u64(d_dsrc)[n - m:] == DSRC_CANARY).all() and (_u64(d_dfirst)[n - m:] == DFIRST_CANARY).all()
    assert np.array_equal(d_canon.cpu().numpy(), canon) and np.array_equal(_u64(d_hash), hashes) and np.array_equal(_u64(d_fs), fs)


# ---- the streaming path ------------------------------------------------------------------------------------------------------
def test_streaming_batches_through_one_table(ctx):
    """Three batches through one persistent table (reset, then insert + lookup with a growing base_index): duplicates cross
    the batches, and the third batch holds only duplicates of the first two."""
    from oracle import oracle as O
    rng = np.random.default_rng(71)
    sizes = (3000, 2500, 1200)
    keys = rng.integers(0, 2 ** 63, size=4000, dtype=np.uint64)
    h1 = keys[rng.integers(0, 2000, size=sizes[0])]
    h2 = keys[rng.integers(1000, 4000, size=sizes[1])]
    seen = np.unique(np.concatenate([h1, h2]))
    h3 = seen[rng.integers(0, len(seen), size=sizes[2])]
    fs_all = O.uniq_first_seen(np.concatenate([h1, h2, h3]))
    ctx.uniq_reset(4000)
    base = 0
    for k, h in enumerate((h1, h2, h3)):
        n = len(h)
        data, offs = MS.batch(rng, rng.integers(0, 41, size=n))
        fs = fs_all[base:base + n]
        b = Buffers(data, offs, np.zeros(n, dtype=np.uint64), out_shift=k + 1, lead=k)
        d_hash = _to(_i64(h))
        ctx.uniq_insert_device(d_hash, n, base)
        ctx.uniq_lookup_device(d_hash, n, b.d_fs)
        b.launch(ctx, base)
        b.fs = fs                                                               # what the lookup must have written, and the compact left alone
        exp = UR.compact(data, offs, fs, base)
        m, B = ctx.uniq_compact_status()
        assert (m, B) == (len(exp[2]), len(exp[0])), k
        UR.assert_equal(b.result(m, B), exp, "batch %d" % k)
        if k == 1:
            assert 0 < m < n and (exp[4] < base).any() and (exp[4] >= base).any()         # duplicates inside the batch and across
        if k == 2:
            assert m == 0 and len(exp[3]) == n and (exp[4] < base).all()
        base += n
    ctx.uniq_status()


# ---- the chain to ORFs -------------------------------------------------------------------------------------------------------
def test_chain_reads_to_orfs(ctx):
    """2 000 rolling-circle reads, a quarter of them copies of earlier reads: monomerize -> monomer compact -> canonicalize ->
    resolve -> uniq compact -> ORFs of the unique canonical monomers.  Nothing but the status calls' totals comes home between
    the steps."""
    import torch
    import circkit_amd
    from oracle import oracle as O
    from tests import orfs_ref
    n = 2000
    data, offs = S.rolling(33, [1000] * n)
    data = data.copy().reshape(n, 1000)
    rng = np.random.default_rng(34)
    for i in range(4, n, 4):
        data[i] = data[int(rng.integers(0, i))]
    data = data.reshape(-1)
    params = dict(seed_len=10, min_identity=0.95)
    # the CPU side
    ends = R.batch(data, offs, threads=16, **params)
    mono, moff, msrc, _ = MR.compact(data, offs, ends)
    canon, hashes = O.canonicalize_batch(mono, moff, True, True, threads=16)
    fs = O.uniq_first_seen(hashes)
    u = UR.compact(canon, moff, fs)
    eo, e = orfs_ref.orfs_batch(u[0], u[1], threads=16)
    assert len(msrc) > 0.05 * n and 0.5 * len(msrc) < len(u[2]) < 0.9 * len(msrc) and len(e) > 0
    # the device side
    nb = len(data)
    dev = _dev()
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
    d_dsrc = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    d_dfirst = torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    ctx.canonicalize_batch_device(d_mono, d_moff, m, out_bytes=d_canon, out_xxh3=d_hash)
    ctx.uniq_resolve_device(d_hash, m, 0, d_fs)
    ctx.uniq_compact_device(d_canon, d_moff, m, d_fs, d_uniq, d_uoff, d_usrc, d_dup_src=d_dsrc, d_dup_first=d_dfirst)
    ctx.uniq_status()
    m2, B2 = ctx.uniq_compact_status()
    cap = 2 * B2 + 16
    d_orf_off = torch.zeros(m2 + 1, dtype=torch.int64, device=dev)
    d_orfs = torch.zeros(cap * 24, dtype=torch.uint8, device=dev)
    ctx.orfs_batch_device(d_uniq, d_uoff, m2, d_orf_off, d_orfs, cap)
    total = ctx.orfs_status()
    # compare
    assert (m, B) == (len(msrc), len(mono)) and (m2, B2) == (len(u[2]), len(u[0]))
    assert np.array_equal(d_mono.cpu().numpy()[:B], mono) and np.array_equal(_u64(d_msrc, m), msrc)
    UR.assert_equal((d_uniq.cpu().numpy()[:B2], _u64(d_uoff, m2 + 1), _u64(d_usrc, m2), _u64(d_dsrc, m - m2), _u64(d_dfirst, m - m2)), u, "chain")
    assert total == len(e) and np.array_equal(_u64(d_orf_off), eo)
    assert np.array_equal(d_orfs.cpu().numpy().view(circkit_amd.api.ORF_DTYPE)[:total], e)


# ---- the host form -----------------------------------------------------------------------------------------------------------
def written_by(recs, res, canonical_out):
    """The FASTA and the table `circkit uniq` writes, from the host form's result."""
    from oracle import oracle as O
    out, out_off, out_src, fs = res
    fasta = b"".join(b">" + recs[int(i)][0] + b"\n" + (bytes(out[int(out_off[j]):int(out_off[j + 1])]) if canonical_out else recs[int(i)][1]) + b"\n"
                     for j, i in enumerate(out_src))
    ids = [O.record_id(h) for h, _ in recs]
    rows = [O.csv_row([ids[int(f)], ids[i]], b",") for i, f in enumerate(fs) if int(f) != i]
    return fasta, (b"id,duplicate_id\n" + b"".join(rows)) if rows else b""


@pytest.mark.parametrize("name", ("repeated", "multiple_sequences", "simple"))
def test_host_form_on_the_cli_fixtures(ctx, name):
    import circkit_amd
    from oracle import oracle as O
    text = open(os.path.join(S.EXAMPLES, name, "in.fasta"), "rb").read()
    recs, data, offs, _ = circkit_amd.api.fasta_parse(text)
    for canonical_out in (False, True):
        exp = O.cli_uniq(text, canonical_out=canonical_out)
        for form in (ctx.uniq_batch, circkit_amd.uniq_batch):
            res = form(data, offs, canonicalize=canonical_out)
            assert written_by(recs, res, canonical_out) == exp, (name, canonical_out)
            if not canonical_out:                               # the batch holds the records normalized
                assert np.array_equal(res[0], UR.compact(data, offs, res[3])[0])
            assert np.array_equal(res[2], np.nonzero(UR.keep_mask(res[3]))[0])
    m = len(res[2])
    assert ctx.uniq_compact_status() == (m, int(res[1][m]))


def test_host_form_on_the_planted_set(ctx, planted):
    data, offs, canon, hashes, fs = planted
    for canonical_out, payload in ((True, canon), (False, data)):
        exp = UR.compact(payload, offs, fs)
        out, out_off, out_src, got_fs = ctx.uniq_batch(data, offs, canonicalize=canonical_out)
        assert np.array_equal(got_fs, fs)
        UR.assert_equal((out, out_off, out_src), exp[:3], "host form, canonicalize=%r" % canonical_out)
        assert ctx.uniq_compact_status() == (len(exp[2]), len(exp[0]))


def test_host_form_empty_batch_and_refusals(ctx):
    import circkit_amd
    for canonical_out in (False, True):
        out = ctx.uniq_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), canonicalize=canonical_out)
        assert [len(x) for x in out] == [0, 1, 0, 0] and int(out[1][0]) == 0 and ctx.uniq_compact_status() == (0, 0)
    out = ctx.uniq_batch(np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.uint64))            # three empty records: one is kept
    assert out[1].tolist() == [0, 0] and out[2].tolist() == [0] and out[3].tolist() == [0, 0, 0]
    with pytest.raises(circkit_amd.CirckitError) as e:
        ctx.uniq_batch(np.zeros(16, dtype=np.uint8), np.array([1, 5], dtype=np.uint64))
    assert e.value.code == -1 and "offsets[0]" in str(e.value)
    with pytest.raises(circkit_amd.CirckitError) as e:
        ctx.uniq_batch(np.zeros(16, dtype=np.uint8), np.array([0, 9, 5], dtype=np.uint64))
    assert e.value.code == -1 and "decrease" in str(e.value)
