"""GPU: circkit_monomers_compact_device / _status / circkit_monomers_batch against the restatement tests/monomers_ref.py, and
the chain monomerize -> compact -> canonicalize -> uniq against the CPU side.  Every record, byte and index is compared;
canaries surround every device output."""
import ctypes
import random

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S
from tests import monomers_ref as MR
from tests import monomers_sets as MS
from tests.test_monomers_compact_cpu import SCAN_COUNTS

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
OFF_CANARY, SRC_CANARY, END_CANARY = 0x25A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 0x43C3C3C3


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


class Buffers:
    """A batch on the device: the payload at in_shift mod 16 behind `lead` canary bytes (offsets[0] = lead), the output at
    out_shift mod 16, canaries round the payload and every output."""

    def __init__(self, data, offs, ends, full_len=None, in_shift=0, out_shift=0, lead=0):
        import torch
        self.n = n = len(offs) - 1
        self.nb = nb = len(data)
        self.data = data
        self.lead = lead
        raw = np.full(GUARD + in_shift + lead + nb + GUARD, IN_CANARY, dtype=np.uint8)
        raw[GUARD + in_shift + lead:GUARD + in_shift + lead + nb] = data
        self.raw_in = raw
        self.d_raw = _to(raw)
        self.d_bytes = self.d_raw[GUARD + in_shift:]
        self.d_offs = _to(_i64(np.asarray(offs, dtype=np.uint64) + np.uint64(lead)))
        self.d_end = _to(np.asarray(ends, dtype=np.uint32).view(np.int32))
        self.d_full = _to(_i64(full_len)) if full_len is not None else None
        self.d_raw_out = torch.full((GUARD + out_shift + nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        self.o0 = GUARD + out_shift
        self.d_out = self.d_raw_out[self.o0:]
        self.d_out_off = torch.full((GUARD + n + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
        self.d_out_src = torch.full((GUARD + n + GUARD,), SRC_CANARY, dtype=torch.int64, device=_dev())
        self.d_kept = torch.full((GUARD + n + GUARD,), END_CANARY, dtype=torch.int32, device=_dev())
        assert self.d_bytes.data_ptr() % 16 == in_shift % 16 and self.d_out.data_ptr() % 16 == out_shift % 16

    def launch(self, ctx, want_kept=True, **flt):
        ctx.monomers_compact_device(self.d_bytes, self.d_offs, self.n, self.d_end, self.d_out, self.d_out_off[GUARD:], self.d_out_src[GUARD:],
                                    d_full_len=self.d_full, d_kept_end=self.d_kept[GUARD:] if want_kept else None, **flt)

    def result(self, m, B, want_kept=True):
        """(out_data, out_offsets, out_src, kept_end) after the canary checks."""
        n = self.n
        raw_out = self.d_raw_out.cpu().numpy()
        out_off = self.d_out_off.cpu().numpy().view(np.uint64)
        out_src = self.d_out_src.cpu().numpy().view(np.uint64)
        kept = self.d_kept.cpu().numpy().view(np.uint32)
        assert np.array_equal(self.d_raw.cpu().numpy(), self.raw_in), "the compact wrote into its input"
        assert (raw_out[:self.o0] == OUT_CANARY).all() and (raw_out[self.o0 + B:] == OUT_CANARY).all(), "wrote outside [out, out + B)"
        assert (out_off[:GUARD] == OFF_CANARY).all() and (out_off[GUARD + m + 1:] == OFF_CANARY).all(), "out_offsets written beyond entry m"
        assert (out_src[:GUARD] == SRC_CANARY).all() and (out_src[GUARD + m:] == SRC_CANARY).all(), "out_src written beyond entry m - 1"
        if want_kept:
            assert (kept[:GUARD] == END_CANARY).all() and (kept[GUARD + n:] == END_CANARY).all(), "kept_end written outside its n entries"
        else:
            assert (kept == END_CANARY).all(), "kept_end written though not asked for"
        assert int(out_off[GUARD + m]) == B
        return (raw_out[self.o0:self.o0 + B].copy(), out_off[GUARD:GUARD + m + 1].copy(), out_src[GUARD:GUARD + m].copy(),
                kept[GUARD:GUARD + n].copy())


def run_device(ctx, data, offs, ends, full_len=None, in_shift=0, out_shift=0, lead=0, want_kept=True, **flt):
    b = Buffers(data, offs, ends, full_len, in_shift, out_shift, lead)
    b.launch(ctx, want_kept, **flt)
    m, B = ctx.monomers_status()
    return b.result(m, B, want_kept)


def check(ctx, case, **place):
    name, data, offs, ends, full_len, flt = case
    exp = MR.compact(data, offs, ends, full_len, **flt)
    got = run_device(ctx, data, offs, ends, full_len, **place, **flt)
    k = 4 if place.get("want_kept", True) else 3                 # without d_kept_end there is no fourth output
    MR.assert_equal(got[:k], exp[:k], (name, place))
    return exp


# ---- the emulator sets ---------------------------------------------------------------------------------------------------
def test_emulator_sets(ctx):
    tile = MS.constants()["TILE_BYTES"]
    for k, s in enumerate(MS.emulator_sets(tile)):
        check(ctx, s)
        check(ctx, s, in_shift=(3 * k + 1) % 16, out_shift=(5 * k + 7) % 16, lead=(7 * k) % 37)


def test_tile_boundary_on_a_record_boundary_at_every_output_shift(ctx):
    rng = np.random.default_rng(5)
    T = MS.constants()["TILE_BYTES"]
    for a in (0, 1, 8, 15):
        for d in (-1, 0, 1):
            first = T - a + d
            check(ctx, MS.case("tile end", rng, [first, 3, 0, 70], [first, 3, 0, 70]), out_shift=a, in_shift=(a + 5) % 16)


def test_decide_on_random_triples(ctx):
    rng = np.random.default_rng(12)
    n = 4000
    lengths = rng.integers(0, 40, size=n)
    ends = rng.integers(0, 45, size=n).astype(np.uint32)
    ends[rng.random(n) < 0.2] = MR.NONE
    full = (lengths + rng.integers(0, 5, size=n)).astype(np.uint64)
    data, offs = MS.batch(rng, lengths, b"ACGT")
    for flt in (dict(), dict(keep_all=True), dict(min_length=10, max_length=30), dict(min_overlap=7), dict(min_overlap_percent=0.51),
                dict(min_overlap_percent=1.0, keep_all=True), dict(min_length=3, min_overlap=2, min_overlap_percent=0.25, max_length=38)):
        check(ctx, ("random", data, offs, ends, full, flt))
        check(ctx, ("random, no kept_end", data, offs, ends, full, flt), want_kept=False)


# ---- device views ------------------------------------------------------------------------------------------------------
def test_device_views(ctx):
    """Every shift mod 16 of the input pointer with a fixed output pointer, every shift of the output pointer with a fixed
    input pointer, four mixed pairs, and offsets[0] != 0."""
    s = MS.misalignment_set()
    for i in range(16):
        check(ctx, s, in_shift=i, out_shift=0)
        check(ctx, s, in_shift=0, out_shift=i)
    for i, o in ((1, 15), (15, 1), (7, 9), (13, 13)):
        check(ctx, s, in_shift=i, out_shift=o, lead=i + o)
    for lead in (1, 16, 1000):
        check(ctx, s, lead=lead)


# ---- the scan's edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", SCAN_COUNTS)
def test_scan_edges(ctx, count):
    """Record counts round every edge of the decide and scan kernels (tests/test_monomers_compact_cpu.py derives the list from
    the kernel's constants), records of 0..3 bytes, a seeded written mask through a crafted d_end, keep_all on and off."""
    rng = np.random.default_rng(count)
    lengths = rng.integers(0, 4, size=count)
    data, offs = MS.batch(rng, lengths, b"ACGT")
    ends = np.where(rng.random(count) < 0.5, rng.integers(0, 4, size=count), MR.NONE).astype(np.uint32)     # some beyond their record
    for keep_all in (False, True):
        exp = check(ctx, ("scan %d" % count, data, offs, ends, None, dict(keep_all=keep_all)), out_shift=count % 16)
        assert len(exp[2]) == count if keep_all else 0 < len(exp[2]) < count or count == 1


# ---- the filters at their boundaries ---------------------------------------------------------------------------------------
def test_filters_at_their_boundaries(ctx):
    for name, lengths, ends, full_len, flt, kept in MS.filter_boundary_cases():
        data, offs = MS.batch(np.random.default_rng(1), lengths)
        e, f = np.array(ends, dtype=np.uint32), np.array(full_len, dtype=np.uint64)
        exp = check(ctx, (name, data, offs, e, f, flt))
        assert (int(exp[3][0]) != MR.NONE) == kept, name
        assert len(exp[2]) == int(kept), name
        check(ctx, (name, data, offs, e, f, dict(flt, keep_all=True)))


def test_ends_beyond_their_records_between_good_ones(ctx):
    """end > n is None before any address is formed from it; end == n writes the whole record."""
    rng = np.random.default_rng(3)
    lengths = [50, 0, 7, 300, 16, 1, 90]
    data, offs = MS.batch(rng, lengths)
    ends = np.array([50, 1, 0xFFFFFFFE, 301, 16, 2, 90], dtype=np.uint32)
    for keep_all in (False, True):
        exp = check(ctx, ("beyond", data, offs, ends, None, dict(keep_all=keep_all)), lead=5, out_shift=3)
        assert exp[3].tolist() == [50, MR.NONE, MR.NONE, MR.NONE, 16, MR.NONE, 90]


# ---- long and lopsided -----------------------------------------------------------------------------------------------------
def test_long_monomers_between_single_bytes(ctx):
    rng = np.random.default_rng(8)
    lengths = [1, 100_000 + 77, 1, 1, 2_000_000 + 1, 1]
    written = [1, 100_000, None, 1, 2_000_000, 1]
    for place in (dict(), dict(in_shift=5, out_shift=11, lead=3)):
        check(ctx, MS.case("long", rng, lengths, written), **place)
        check(ctx, MS.case("long, keep_all", rng, lengths, written, keep_all=True), **place)


def test_only_the_last_record_is_written(ctx):
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 2000, size=3000).tolist()
    check(ctx, MS.case("last only", rng, lengths, [None] * 2999 + [lengths[-1] // 2 + 1]), out_shift=9)
    lengths[-1] = 0
    check(ctx, MS.case("last only, empty", rng, lengths, [None] * 2999 + [0]))


# ---- the chain -------------------------------------------------------------------------------------------------------------
def chain_on_device(ctx, data, offs, params, flt):
    """monomerize -> compact -> status -> canonicalize (bytes + xxh3) -> uniq resolve, all on the device: per output record
    (canonical bytes, offsets, out_src, hash, first_seen), and kept_end."""
    import torch
    n, nb = len(offs) - 1, len(data)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_end = torch.empty(n, dtype=torch.int32, device=_dev())
    d_mono = torch.empty(max(nb, 1), dtype=torch.uint8, device=_dev())
    d_moff = torch.empty(n + 1, dtype=torch.int64, device=_dev())
    d_src = torch.empty(n, dtype=torch.int64, device=_dev())
    d_kept = torch.empty(n, dtype=torch.int32, device=_dev())
    ctx.monomerize_batch_device(d_bytes, d_offs, n, d_end, **params)
    ctx.monomers_compact_device(d_bytes, d_offs, n, d_end, d_mono, d_moff, d_src, d_kept_end=d_kept, **flt)
    m, B = ctx.monomers_status()
    d_canon = torch.empty(max(B, 1), dtype=torch.uint8, device=_dev())
    d_hash = torch.empty(max(m, 1), dtype=torch.int64, device=_dev())
    d_fs = torch.empty(max(m, 1), dtype=torch.int64, device=_dev())
    ctx.canonicalize_batch_device(d_mono, d_moff, m, out_bytes=d_canon, out_xxh3=d_hash)
    ctx.uniq_resolve_device(d_hash, m, 0, d_fs)
    ctx.uniq_status()
    u64 = lambda t, k: t.cpu().numpy().view(np.uint64)[:k]
    return (d_mono.cpu().numpy()[:B], d_canon.cpu().numpy()[:B], u64(d_moff, m + 1), u64(d_src, m), u64(d_hash, m), u64(d_fs, m),
            d_kept.cpu().numpy().view(np.uint32))


def chain_on_cpu(data, offs, params, flt):
    from oracle import oracle as O
    ends = R.batch(data, offs, threads=16, **params)
    mono, moff, src, kept = MR.compact(data, offs, ends, **flt)
    canon, hashes = O.canonicalize_batch(mono, moff, True, True, threads=16)
    return mono, canon, moff, src, hashes, O.uniq_first_seen(hashes), kept


def compare_chain(got, exp):
    for name, g, x in zip(("monomer bytes", "canonical bytes", "offsets", "out_src", "xxh3", "first_seen", "kept_end"), got, exp):
        assert len(g) == len(x), (name, len(g), len(x))
        bad = np.nonzero(np.asarray(g) != np.asarray(x))[0]
        assert len(bad) == 0, (name, int(bad[0]), len(bad))


@pytest.fixture(scope="module")
def rolling_batch():
    data, offs = S.rolling(21, [1000] * 200_000)
    params = dict(seed_len=10, min_identity=0.95)
    return data, offs, params, chain_on_cpu(data, offs, params, {})


def test_chain_rolling(ctx, rolling_batch):
    """200 000 x 1 kb rolling-circle records, seed 10, identity 0.95."""
    data, offs, params, exp = rolling_batch
    got = chain_on_device(ctx, data, offs, params, {})
    compare_chain(got, exp)
    m = len(exp[3])
    assert 0.05 * len(offs) < m < 0.95 * len(offs) and len(np.unique(exp[5])) == len(np.unique(exp[4]))


def test_chain_mixed_lengths_sensitive(ctx):
    """20 000 records of 200 b .. 20 kb, the sensitive form, --min-overlap-percent 0.51."""
    rng = np.random.default_rng(4)
    lengths = np.exp(rng.uniform(np.log(200), np.log(20000), size=20000)).astype(np.int64)
    d1, o1 = S.rolling(5, lengths[:14000])
    d2, o2 = S.rolling(6, lengths[14000:], pmin=1000, pmax=6000, rate=0.003)
    data = np.concatenate([d1, d2])
    offs = np.concatenate([o1, o2[1:] + o1[-1]])
    params = dict(seed_len=10, min_identity=0.95, sensitive=True)
    flt = dict(min_overlap_percent=0.51)
    exp = chain_on_cpu(data, offs, params, flt)
    compare_chain(chain_on_device(ctx, data, offs, params, flt), exp)
    assert 0.05 * 20000 < len(exp[3]) < 0.95 * 20000


# ---- the host form ---------------------------------------------------------------------------------------------------------
def test_host_form_on_the_rolling_batch(ctx, rolling_batch):
    data, offs, params, exp = rolling_batch
    got = ctx.monomers_batch(data, offs, **params)
    MR.assert_equal(got, (exp[0], exp[2], exp[3], exp[6]), "host form, rolling")
    assert ctx.monomers_status() == (len(exp[3]), len(exp[0]))


def test_host_form_equals_device_form_on_the_adversarial_set(ctx):
    import circkit_amd
    seqs = S.adversarial()
    data, offs = S.pack(seqs)
    full = np.array([len(s) + (i % 3) for i, s in enumerate(seqs)], dtype=np.uint64)
    for params, flt in ((dict(seed_len=10, min_identity=0.9), dict()), (dict(seed_len=5, max_mismatch=1, sensitive=True), dict(keep_all=True)),
                        (dict(seed_len=10, min_identity=0.95), dict(min_length=200, max_length=1100, min_overlap=100)),
                        (dict(seed_len=10, max_mismatch=5), dict(min_overlap_percent=1.0, keep_all=True))):
        ends = ctx.monomerize_batch(data, offs, **params)
        assert np.array_equal(ends, R.batch(data, offs, threads=16, **params))
        exp = MR.compact(data, offs, ends, full, **flt)
        MR.assert_equal(run_device(ctx, data, offs, ends, full, in_shift=3, out_shift=6, **flt), exp, ("device", params, flt))
        MR.assert_equal(ctx.monomers_batch(data, offs, full_len=full, **params, **flt), exp, ("host", params, flt))
    got = circkit_amd.monomers_batch(data, offs, seed_len=10, min_identity=0.9)          # the module-level form, default context
    MR.assert_equal(got, MR.compact(data, offs, R.batch(data, offs, seed_len=10, min_identity=0.9)), "module level")


def test_host_form_refuses_a_record_of_2_32_symbols(ctx):
    import circkit_amd
    offs = np.array([0, 5, 5 + 2 ** 32], dtype=np.uint64)
    with pytest.raises(circkit_amd.CirckitError) as e:
        ctx.monomers_batch(np.zeros(16, dtype=np.uint8), offs)
    assert e.value.code == -4
    with pytest.raises(circkit_amd.CirckitError) as e:
        ctx.monomers_batch(np.zeros(16, dtype=np.uint8), np.array([1, 5], dtype=np.uint64))
    assert e.value.code == -1 and "offsets[0]" in str(e.value)


# ---- batch sizes and stream order ------------------------------------------------------------------------------------------
def test_empty_batches(ctx):
    import torch
    # n = 0 with an offsets buffer: out_offsets[0] = 0 is written, nothing else
    d_out_off = torch.full((4,), OFF_CANARY, dtype=torch.int64, device=_dev())
    d_one = torch.zeros(1, dtype=torch.int64, device=_dev())
    ctx.monomers_compact_device(None, d_one, 0, None, None, d_out_off, None)
    assert ctx.monomers_status() == (0, 0)
    assert d_out_off.cpu().numpy().tolist() == [0, OFF_CANARY, OFF_CANARY, OFF_CANARY]
    ctx.monomers_compact_device(None, None, 0, None, None, None, None)
    assert ctx.monomers_status() == (0, 0)
    out = ctx.monomers_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    assert [len(x) for x in out] == [0, 1, 0, 0] and ctx.monomers_status() == (0, 0)
    # m = 0: no record is written
    rng = np.random.default_rng(2)
    got = check(ctx, MS.case("m = 0", rng, [10, 0, 300], [None, None, None]))
    assert len(got[0]) == 0 and got[1].tolist() == [0]
    # records, but no bytes
    check(ctx, MS.case("B = 0", rng, [10, 0, 300], [0, 0, None]))
    check(ctx, MS.case("no payload", rng, [0, 0, 0], [0, None, 0], keep_all=True))


def test_back_to_back_compacts_on_one_stream(ctx):
    """Two compacts of one batch with different filters, no synchronise between them: both results are right and the status
    reports the second's totals."""
    rng = np.random.default_rng(31)
    lengths = rng.integers(0, 3000, size=5000)
    data, offs = MS.batch(rng, lengths, b"ACGT")
    ends = np.where(rng.random(5000) < 0.6, (lengths * rng.random(5000)).astype(np.int64), MR.NONE).astype(np.uint32)
    a, b = Buffers(data, offs, ends, out_shift=4), Buffers(data, offs, ends, in_shift=9)
    fa, fb = dict(min_length=500), dict(keep_all=True, max_length=1500)
    a.launch(ctx, **fa)
    b.launch(ctx, **fb)
    ea, eb = MR.compact(data, offs, ends, **fa), MR.compact(data, offs, ends, **fb)
    assert ctx.monomers_status() == (len(eb[2]), len(eb[0]))
    assert (len(ea[2]), len(ea[0])) != (len(eb[2]), len(eb[0]))
    MR.assert_equal(a.result(len(ea[2]), len(ea[0])), ea, "first of two")
    MR.assert_equal(b.result(len(eb[2]), len(eb[0])), eb, "second of two")


# ---- the refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_ctx_usable(ctx):
    import circkit_amd
    rng = np.random.default_rng(41)
    case = MS.case("after a refusal", rng, [40, 100, 7], [20, None, 7])
    _, data, offs, ends, _, _ = case
    b = Buffers(data, offs, ends)
    args = dict(d_bytes=b.d_bytes, d_offsets=b.d_offs, n_records=b.n, d_end=b.d_end, d_out_bytes=b.d_out, d_out_offsets=b.d_out_off[GUARD:],
                d_out_src=b.d_out_src[GUARD:])

    def refused(message, **change):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.monomers_compact_device(**dict(args, **change))
        assert e.value.code == -1 and message in str(e.value), str(e.value)
        check(ctx, case)                                        # the next valid call works

    with pytest.raises(circkit_amd.CirckitError) as e:          # a null filter: past the Python constructor, on the C ABI itself
        ctx._check(ctx._lib.circkit_monomers_compact_device(ctx._h, b.d_bytes.data_ptr(), b.d_offs.data_ptr(), b.n, b.d_end.data_ptr(), None,
                                                            None, b.d_out.data_ptr(), b.d_out_off[GUARD:].data_ptr(),
                                                            b.d_out_src[GUARD:].data_ptr(), None))
    assert e.value.code == -1 and "null filter" in str(e.value)
    check(ctx, case)
    for name in ("d_bytes", "d_offsets", "d_end", "d_out_bytes", "d_out_offsets", "d_out_src"):
        refused("null buffer", **{name: None})
    # An output whose owed room (as many bytes as the payload) overlaps the input payload.  The offsets are the device's, so
    # the device refuses: no record is written, the totals are 0 and the status carries the error.  An output that ends where
    # the payload begins, or begins where it ends, does not overlap.
    import torch
    nb = b.nb
    whole = torch.full((GUARD + 3 * nb + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    whole[GUARD + nb:GUARD + 2 * nb] = _to(data)
    before = whole.cpu().numpy().copy()
    d_offs = _to(_i64(offs))
    exp = MR.compact(data, offs, ends)
    for out0, overlaps in ((GUARD, False), (GUARD + 1, True), (GUARD + nb, True), (GUARD + 2 * nb - 1, True), (GUARD + 2 * nb, False)):
        ctx.monomers_compact_device(whole[GUARD + nb:], d_offs, b.n, b.d_end, whole[out0:], b.d_out_off[GUARD:], b.d_out_src[GUARD:])
        if overlaps:
            with pytest.raises(circkit_amd.CirckitError) as e:
                ctx.monomers_status()
            assert e.value.code == -1 and "overlaps" in str(e.value)
            assert np.array_equal(whole.cpu().numpy(), before), "an overlapping output was written"
            check(ctx, case)
        else:
            m, B = ctx.monomers_status()
            assert (m, B) == (len(exp[2]), len(exp[0]))
            now = whole.cpu().numpy()
            assert np.array_equal(now[out0:out0 + B], exp[0])
            now[out0:out0 + B] = OUT_CANARY
            assert np.array_equal(now, before), "wrote outside [out, out + B), or into the payload"
            whole[out0:out0 + B] = OUT_CANARY
