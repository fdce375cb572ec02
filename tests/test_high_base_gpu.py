"""GPU: every batch unit with its payload round byte 2^32 of one big device buffer (run with -m gpu).

The input sets and yardsticks are the units' own; what is new is where the payload lies: tests/high_base.py places each set so
that its record j straddles byte 2^32 of `big` ("middle") or starts exactly on it ("boundary"), passes `big` as d_bytes with the
absolute offsets, and every output must equal, exactly, the answer the yardstick gives for the same set with offsets from 0.  The
alias region big[0, 4 MiB) holds a decoy that differs from the payload at every position above the line, so a payload position
truncated to 32 bits reads a wrong byte.  After each call the 8 MiB window round the line and the decoy must be unchanged.
Only those 12 MiB of the 4 GiB + 8 MiB are ever written.  The last section places an output 4 GiB below a payload that lies above
the line (same low 32 bits: must be accepted) and on the payload's last 16 bytes (must be refused)."""
import numpy as np
import pytest

from tests import high_base as H

pytestmark = pytest.mark.gpu

LINE, HALF = H.LINE, H.HALF
GUARD = 64
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
C64, C32, C8 = 0x25A5A5A5A5A5A5A5, 0x3F3F3F3F, 0xEE
OK, INVALID_ARG = 0, -1


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


class High:
    """The big buffer, the decoy and the window as they must be, and the ctx (on torch's stream)."""

    def __init__(self):
        import circkit_amd
        import torch
        self.ctx = circkit_amd.Context(0)
        self.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.big = torch.empty(H.BIG, dtype=torch.uint8, device=_dev())
        self.low, self.win, self.top = self.big[:HALF], self.big[LINE - HALF:LINE + HALF], self.big[LINE + HALF:]
        self.dec0 = H.decoy(1, HALF)
        self.d_dec = _to(self.dec0)
        self.d_win = torch.full((2 * HALF,), IN_CANARY, dtype=torch.uint8, device=_dev())
        self.top.fill_(C8)

    def put(self, data, absolute):
        """The payload at big[absolute[0] ...], canaries round it in the window, the decoy made to differ under it; returns the
        absolute offsets on the device."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        p0 = int(absolute[0])
        assert LINE - HALF <= p0 and p0 + len(data) <= LINE + HALF and int(absolute[-1]) - p0 == len(data)
        self.d_win.fill_(IN_CANARY)
        if len(data):
            self.d_win[p0 - (LINE - HALF):p0 - (LINE - HALF) + len(data)] = _to(data)
        self.win.copy_(self.d_win)
        self.d_dec.copy_(_to(H.differing(self.dec0, data, absolute)))
        self.low.copy_(self.d_dec)
        return _to(_i64(absolute))

    def unchanged(self, what=""):
        import torch
        assert torch.equal(self.win, self.d_win), ("the call wrote into the window round the line", what)
        assert torch.equal(self.low, self.d_dec), ("the call wrote into the decoy", what)

    def close(self):
        self.ctx.close()
        del self.big, self.low, self.win, self.top


@pytest.fixture(scope="module")
def hb():
    import torch
    h = High()
    yield h
    h.close()
    torch.cuda.empty_cache()


def canaried(n, dtype, value):
    import torch
    return torch.full((GUARD + n + GUARD,), value, dtype=dtype, device=_dev())


def opened(t, n, value, dtype):
    """The n entries between the canaries of a tensor made by canaried(), after checking the canaries."""
    a = t.cpu().numpy().view(dtype)
    assert (a[:GUARD] == value).all() and (a[GUARD + n:] == value).all(), "written outside the n entries"
    return a[GUARD:GUARD + n].copy()


def placements(offs, j, extra=()):
    return [(m, 0, H.place(offs, j, m)) for m in H.MODES] + [("boundary", at, H.place(offs, j, "boundary", at)) for at in extra]


# ---- sketch and anchors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("lengths", "symbols"))
@pytest.mark.parametrize("k,lb", H.SKETCH_PARAMS)
def test_sketch_and_anchors(hb, kind, k, lb):
    """Positions above the line: the input offsets of every record behind j, and the spans of record j (3 spans and a tail: in
    "middle" the line lies inside the second, in the third placement exactly on the second span's start)."""
    import torch
    from tests import prealign_ref as P
    from tests import sketch_sets as S
    from tests.test_sketch_gpu import status
    recs, j, seg = H.sketch_records(kind, k)
    data, offs = H.pack(recs)
    n, bins = len(recs), 1 << lb
    exp_rows, exp_counts = S.expected(recs, k, lb)
    a_rows, a_counts, a_anc = P.anchors_batch(recs, k, lb)
    assert np.array_equal(a_rows, exp_rows) and np.array_equal(a_counts, exp_counts)     # (the two yardsticks agree)
    for mode, at, absolute in placements(offs, j, (seg,)):
        d_offs = hb.put(data, absolute)
        for anchors in (False, True):
            d_rows, d_counts, d_anc = canaried(n * bins, torch.int64, C64), canaried(n, torch.int32, C32), canaried(n * bins, torch.int32, C32)
            if anchors:
                hb.ctx.sketch_anchors_device(hb.big, d_offs, n, d_rows[GUARD:], d_anc[GUARD:], d_counts[GUARD:], k=k, log2_bins=lb)
            else:
                hb.ctx.sketch_batch_device(hb.big, d_offs, n, d_rows[GUARD:], d_counts[GUARD:], k=k, log2_bins=lb)
            what = (kind, k, lb, mode, at, anchors)
            assert status(hb.ctx) == (OK, int(exp_counts.sum()), 0), what
            hb.unchanged(what)
            assert np.array_equal(opened(d_counts, n, C32, np.uint32), exp_counts), what
            assert np.array_equal(opened(d_rows, n * bins, C64, np.uint64).reshape(n, bins), exp_rows), what
            anc = opened(d_anc, n * bins, C32, np.uint32)
            assert np.array_equal(anc.reshape(n, bins), a_anc) if anchors else (anc == C32).all(), what
            assert np.array_equal(d_offs.cpu().numpy().view(np.uint64), absolute)


# ---- monomerize --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed_len", (5, 63))
def test_monomerize(hb, seed_len):
    """Positions above the line: the input offsets behind the 2 x 1100 dimer, whose second copy starts on the line ("middle") --
    the count from the end and the sensitive count from the front both cross it -- or whose first byte does ("boundary")."""
    import torch
    from tests import mono_ref as R
    from tests import mono_sets as S
    recs, j = H.mono_records()
    data, offs = H.pack(recs)
    n = len(recs)
    settings = S.settings((seed_len,))
    expected = [R.batch(data, offs, threads=16, **kw) for kw in settings]
    assert sum(int((e != R.NONE).sum()) for e in expected) > 1000
    for mode, at, absolute in placements(offs, j):
        d_offs = hb.put(data, absolute)
        for kw, exp in zip(settings, expected):
            d_end = canaried(n, torch.int32, C32)
            hb.ctx.monomerize_batch_device(hb.big, d_offs, n, d_end[GUARD:], **kw)
            hb.ctx.synchronize()
            got = opened(d_end, n, C32, np.uint32)
            hb.unchanged((kw, mode))
            bad = np.flatnonzero(got != exp)
            assert len(bad) == 0, (kw, mode, bad[:5].tolist(), [len(recs[i]) for i in bad[:5]], got[bad[:5]].tolist(), exp[bad[:5]].tolist())


# ---- the monomer compact -------------------------------------------------------------------------------------------------------
def test_monomers_compact(hb):
    """Positions above the line: the input offsets from record j on.  The outputs are small tensors; kept bytes are read from
    both sides of the line into one output."""
    from tests import monomers_ref as MR
    from tests.test_monomers_compact_gpu import Buffers
    ran = 0
    for k, (case, j) in enumerate(H.monomers_cases()):
        name, data, offs, ends, full_len, flt = case
        exp = MR.compact(data, offs, ends, full_len, **flt)
        places = placements(offs, j) if j is not None else [("boundary", 0, H.place(offs, len(offs) - 2, "boundary"))]
        for mode, at, absolute in places:
            b = Buffers(data, offs, ends, full_len, out_shift=(5 * k + 7) % 16)
            b.d_bytes, b.d_offs = hb.big, hb.put(data, absolute)
            b.launch(hb.ctx, **flt)
            m, B = hb.ctx.monomers_status()
            hb.unchanged((name, mode))
            MR.assert_equal(b.result(m, B), exp, (name, mode))
            ran += 1
    assert ran == 2 * len(H.monomers_cases()) - len(H.NO_MIDDLE)


# ---- the uniq compact ----------------------------------------------------------------------------------------------------------
def test_uniq_compact(hb):
    """Positions above the line: the input offsets from record j on and, with base_index = 2^32 + 12345, every global index:
    d_first_seen, what is kept (first_seen == base + i) and d_dup_first."""
    from tests import uniq_compact_ref as UR
    from tests.test_uniq_compact_gpu import Buffers
    for k, (name, data, offs, fs, base, j) in enumerate(H.uniq_cases()):
        exp = UR.compact(data, offs, fs, base)
        assert 0 < len(exp[2]) < H.UNIQ_COUNT and (not base or (exp[4] > 2 ** 32).any())
        for mode, at, absolute in placements(offs, j):
            b = Buffers(data, offs, fs, out_shift=(3 * k + 1) % 16)
            b.d_bytes, b.d_offs = hb.big, hb.put(data, absolute)
            b.launch(hb.ctx, base)
            m, B = hb.ctx.uniq_compact_status()
            hb.unchanged((name, mode))
            assert (m, B) == (len(exp[2]), len(exp[0])), (name, mode, m, B)
            UR.assert_equal(b.result(m, B), exp, (name, mode))


# ---- windows: gather, one window per record, translate ---------------------------------------------------------------------------
WINDOWS, TRANSLATE = H.windows_cases(), H.translate_cases()
_EXPECTED = {}


def expected_once(key, fn):
    if key not in _EXPECTED:
        _EXPECTED[key] = fn()
    return _EXPECTED[key]


@pytest.mark.parametrize("k", range(len(WINDOWS)), ids=[c[0] for c in WINDOWS])
def test_windows_gather(hb, k):
    """Positions above the line: the input offsets from record j on; windows on either strand read from both sides of it, go
    round their record, and start at up to 2^32 - 1."""
    from tests import test_windows_gpu as G
    from tests import windows_ref as R
    name, data, offs, wins, place = WINDOWS[k]
    exp = expected_once(("gather", k), lambda: R.gather(data, offs, wins))
    for mode, at, absolute in placements(offs, H.inner_longest(offs)):
        b = G.Buffers(data, offs, wins, len(exp[0]), out_shift=place.get("out_shift", 0))
        b.d_bytes, b.offs = hb.big, absolute
        b.d_offs = hb.put(data, absolute)
        b.launch(hb.ctx)
        rc, total, bad = G.status(hb.ctx)
        hb.unchanged((name, mode))
        assert (total, bad) == (len(exp[0]), exp[2]) and rc == (INVALID_ARG if exp[2] else OK), (name, mode, rc, total, bad)
        out, off = b.result(total)
        assert np.array_equal(off, exp[1]) and np.array_equal(out, exp[0]), (name, mode)


def test_windows_of_records(hb):
    """Only the offsets are read: absolute ones, on both sides of the line, must give the windows of the lengths."""
    import torch
    from tests import windows_ref as R
    batches = {c[2].tobytes(): c for c in WINDOWS}
    assert len(batches) >= 2
    for name, data, offs, _, _ in batches.values():
        lengths = np.diff(offs.astype(np.int64))
        n = len(lengths)
        for mode, at, absolute in placements(offs, H.inner_longest(offs)):
            d_offs = _to(_i64(absolute))
            for kind, kw in (("rotate_bases", dict(bases=7)), ("rotate_bases", dict(bases=-2 ** 63)), ("rotate_percent", dict(percent=0.37)), ("cat", {}),
                             ("decat", {}), ("revcomp", {})):
                d_win = canaried(24 * n, torch.uint8, OUT_CANARY)
                hb.ctx.windows_of_records_device(d_offs, n, kind, d_win[GUARD:], **kw)
                hb.ctx.synchronize()
                got = opened(d_win, 24 * n, OUT_CANARY, np.uint8).view(R.WINDOW_DTYPE)
                kinds = dict(rotate_bases=R.ROTATE_BASES, rotate_percent=R.ROTATE_PERCENT, cat=R.CAT, decat=R.DECAT, revcomp=R.REVCOMP)
                assert np.array_equal(got, R.windows_of_records(lengths, kinds[kind], **kw)), (name, mode, kind, kw)


@pytest.mark.parametrize("k", range(len(TRANSLATE)), ids=[c[0] for c in TRANSLATE])
def test_windows_translate(hb, k):
    """Positions above the line: the input offsets from record j on; codons are read from both sides of it."""
    from tests import test_translate_gpu as TG
    from tests import translate_sets as TS
    name, data, offs, wins, place, code = TRANSLATE[k]
    exp = expected_once(("translate", k), lambda: TS.expected(TRANSLATE[k]))
    for mode, at, absolute in placements(offs, H.inner_longest(offs)):
        b = TG.Buffers(data, offs, wins, len(exp[0]), out_shift=place.get("out_shift", 0))
        b.d_bytes, b.offs = hb.big, absolute
        b.d_offs = hb.put(data, absolute)
        b.launch(hb.ctx, code)
        rc, total, bad = TG.status(hb.ctx)
        hb.unchanged((name, mode))
        assert (total, bad) == (len(exp[0]), exp[2]) and rc == (INVALID_ARG if exp[2] else OK), (name, mode, rc, total, bad)
        out, off = b.result(total)
        assert np.array_equal(off, exp[1]) and np.array_equal(out, exp[0]), (name, mode)


# ---- FASTA write with a body -----------------------------------------------------------------------------------------------------
class BigBody:
    """Stands where a Run keeps its body image: the body is the big buffer, whose window the test checks itself."""

    def __init__(self, d):
        self.d = d

    def unchanged(self, lo=0, hi=0):
        return True


FASTA_WRITE = H.fasta_write_cases()


@pytest.mark.parametrize("k", range(len(FASTA_WRITE)), ids=[c.name for c in FASTA_WRITE])
def test_fasta_write_with_a_body(hb, k):
    """Positions above the line: d_body_offsets (d_body_offsets[0] >= 2^32 - 4 MiB, the body on both sides of the line); the text,
    its spans and the output are small."""
    from tests import fasta_write_sets as S
    from tests import test_fasta_write_gpu as FW
    c = FASTA_WRITE[k]
    recs, bad = S.expected(c)
    total = sum(len(r) for r in recs)
    data, offs = H.body_of(c)
    for mode, at, absolute in placements(offs, H.inner_longest(offs)):
        assert int(absolute[0]) >= LINE - HALF
        r = FW.Run(c, total)
        r.body, r.d_body_off = BigBody(hb.big), hb.put(data, absolute)
        r.launch(hb.ctx)
        rc, got_total, got_bad, msg = FW.status(hb.ctx)
        hb.unchanged((c.name, mode))
        assert rc == (INVALID_ARG if bad else OK), (c.name, mode, rc, msg)
        text, off = r.result(got_total)
        S.check(c, (text or b"", off, got_total, got_bad, 0), what="%s %s" % (c.name, mode))


# ---- canonicalize, lmsr, xxh3 ------------------------------------------------------------------------------------------------------
class Address:
    """A device address that is no tensor's first byte (what circkit_amd.api._ptr reads)."""

    def __init__(self, a):
        self.a = a

    def data_ptr(self):
        return self.a


@pytest.mark.parametrize("name", sorted(H.canon_sets()))
def test_canonicalize_lmsr_xxh3(hb, name):
    """Positions above the line: the input offsets from record j on, and the output offsets, which are the input's.  d_out_bytes is
    a pointer positioned so that d_out_bytes + offsets[i] is valid: it names no byte itself, d_out_bytes + offsets[0] is
    big[2^32 + 4 MiB + 64], the part of the big buffer behind the window, so that an output position truncated to 32 bits would
    still land inside the allocation (and show as missing bytes) instead of faulting.  Each output set runs three times in a row,
    as in tests/test_canon_lengths_gpu.py: the first call of a set runs on the builds the previous set's mode chose."""
    import torch
    from oracle import oracle as O
    O.lib()
    recs = H.canon_sets()[name]
    data, offs = H.pack(recs)
    n, nb = len(recs), len(data)
    assert nb + 2 * GUARD <= HALF
    exp_b, exp_h, exp_i, exp_s = O.canonicalize_batch_aux(data, offs, True, True, True, True, threads=16)
    lexp_b, lexp_i = O.lmsr_batch(data, offs, threads=16)
    exp_raw = np.array([O.xxh3_64(s) for s in recs], dtype=np.uint64)
    d_top_expect = torch.full((HALF,), C8, dtype=torch.uint8, device=_dev())

    def top_is(expected_bytes, what):
        d_top_expect.fill_(C8)
        if expected_bytes is not None:
            d_top_expect[GUARD:GUARD + nb] = _to(expected_bytes)
        if not torch.equal(hb.top, d_top_expect):
            got = hb.top[GUARD:GUARD + nb].cpu().numpy()
            o = offs.astype(np.int64)
            bad = [i for i in range(n) if expected_bytes is None or not np.array_equal(got[o[i]:o[i + 1]], expected_bytes[o[i]:o[i + 1]])]
            raise AssertionError("%s: bytes of %d records differ, first %s (lengths %s), or bytes outside [offsets[0], offsets[n]) were written"
                                 % (what, len(bad), bad[:5], [len(recs[i]) for i in bad[:5]]))

    for mode, at, absolute in placements(offs, H.inner_longest(offs)):
        d_offs = hb.put(data, absolute)
        out = Address(hb.big.data_ptr() + LINE + HALF + GUARD - int(absolute[0]))
        for outs, lmsr, reps in (("bish", False, 3), ("bh", False, 3), ("b", False, 1), ("h", False, 2), ("bi", True, 2), ("raw", False, 1)):
            for rep in range(reps):
                what = (name, mode, outs, "lmsr" if lmsr else "", rep)
                hb.top.fill_(C8)
                d_idx, d_strand, d_hash = canaried(n, torch.int32, C32), canaried(n, torch.uint8, C8), canaried(n, torch.int64, C64)
                ob = out if "b" in outs else None
                if outs == "raw":
                    hb.ctx.xxh3_batch_device(hb.big, d_offs, n, d_hash[GUARD:])
                    hb.ctx.synchronize()
                elif lmsr:
                    hb.ctx.lmsr_batch_device(hb.big, d_offs, n, out_bytes=ob, out_index=d_idx[GUARD:])
                else:
                    hb.ctx.canonicalize_batch_device(hb.big, d_offs, n, out_bytes=ob, out_index=d_idx[GUARD:] if "i" in outs else None,
                                                     out_strand=d_strand[GUARD:] if "s" in outs else None, out_xxh3=d_hash[GUARD:] if "h" in outs else None)
                if outs != "raw":
                    assert hb.ctx.last_batch_mode() in (1, 2, 3) and hb.ctx.batch_status() == 0, what
                torch.cuda.synchronize()
                hb.unchanged(what)
                top_is((lexp_b if lmsr else exp_b) if ob is not None else None, what)
                idx, strand, hs = opened(d_idx, n, C32, np.uint32), opened(d_strand, n, C8, np.uint8), opened(d_hash, n, C64, np.uint64)
                for key, got, exp, canary in (("i", idx, lexp_i if lmsr else exp_i, C32), ("s", strand, exp_s, C8),
                                              ("h", hs, exp_raw if outs == "raw" else exp_h, C64)):
                    if key in outs or (key == "h" and outs == "raw"):
                        bad = np.flatnonzero(got != exp)
                        assert len(bad) == 0, (what, key, bad[:5].tolist(), [len(recs[i]) for i in bad[:5]])
                    else:
                        assert (got == canary).all(), (what, key, "written although it was not asked for")


# ---- an output with the payload's low 32 bits, and one on its last 16 bytes ------------------------------------------------------
ABOVE = LINE + (1 << 20) + 5                      # the payload of this section starts here: wholly above the line


class Overlap:
    """A payload wholly above the line and the two output places: big[p0 - 2^32 ...], 4 GiB below it with the same low 32 bits,
    which must be accepted and written, and big[p1 - 16 ...], on the payload's last 16 bytes, which must be refused."""

    def __init__(self, hb, data, offs):
        self.hb, self.nb = hb, len(data)
        o = np.asarray(offs, dtype=np.uint64)
        self.absolute = o - o[0] + np.uint64(ABOVE)
        self.d_offs = hb.put(data, self.absolute)
        self.below, self.at_end = ABOVE - LINE, ABOVE + self.nb - 16
        assert self.nb >= 16 and (self.below & 0xFFFFFFFF) == (ABOVE & 0xFFFFFFFF)

    def accepted(self, expected_bytes, what):
        """the decoy but for [below, below + len(expected)), which holds the output; the window as it was"""
        import torch
        hb, lo, hi = self.hb, self.below, self.below + len(expected_bytes)
        assert torch.equal(hb.win, hb.d_win), ("the call wrote into the window round the line", what)
        assert torch.equal(hb.low[:lo], hb.d_dec[:lo]) and torch.equal(hb.low[hi:], hb.d_dec[hi:]), ("wrote outside [out, out + total)", what)
        assert np.array_equal(hb.low[lo:hi].cpu().numpy(), expected_bytes), what
        hb.low.copy_(hb.d_dec)


def test_overlap_monomers_compact(hb):
    import circkit_amd
    from tests import monomers_ref as MR
    from tests import monomers_sets as MS
    from tests.test_monomers_compact_gpu import Buffers
    name, data, offs, ends, full_len, flt = MS.misalignment_set()
    exp = MR.compact(data, offs, ends, full_len, **flt)
    v = Overlap(hb, data, offs)
    b = Buffers(data, offs, ends, full_len)
    hb.ctx.monomers_compact_device(hb.big, v.d_offs, b.n, b.d_end, hb.big[v.below:], b.d_out_off[GUARD:], b.d_out_src[GUARD:], d_kept_end=b.d_kept[GUARD:], **flt)
    m, B = hb.ctx.monomers_status()
    assert (m, B) == (len(exp[2]), len(exp[0]))
    v.accepted(exp[0], "monomers compact, 4 GiB below")
    u64 = lambda t, k: t.cpu().numpy().view(np.uint64)[GUARD:GUARD + k]
    MR.assert_equal((exp[0], u64(b.d_out_off, m + 1), u64(b.d_out_src, m), b.d_kept.cpu().numpy().view(np.uint32)[GUARD:GUARD + b.n]), exp,
                    "monomers compact, 4 GiB below")
    b = Buffers(data, offs, ends, full_len)
    hb.ctx.monomers_compact_device(hb.big, v.d_offs, b.n, b.d_end, hb.big[v.at_end:], b.d_out_off[GUARD:], b.d_out_src[GUARD:], **flt)
    with pytest.raises(circkit_amd.CirckitError) as e:
        hb.ctx.monomers_status()
    assert e.value.code == INVALID_ARG and "overlaps" in str(e.value)
    hb.unchanged("monomers compact, on the payload's last 16 bytes")
    assert (b.d_out_src.cpu().numpy().view(np.uint64) == 0x5A5A5A5A5A5A5A5A).all()


def test_overlap_uniq_compact(hb):
    import circkit_amd
    from tests import uniq_compact_ref as UR
    from tests.test_uniq_compact_gpu import Buffers, DFIRST_CANARY, DSRC_CANARY, SRC_CANARY
    name, data, offs, fs, base, _ = H.uniq_cases()[1]
    assert base > 2 ** 32
    exp = UR.compact(data, offs, fs, base)
    v = Overlap(hb, data, offs)
    b = Buffers(data, offs, fs)
    args = lambda d_out: (hb.big, v.d_offs, b.n, b.d_fs, d_out, b.d_out_off[GUARD:], b.d_out_src[GUARD:])
    hb.ctx.uniq_compact_device(*args(hb.big[v.below:]), base_index=base, d_dup_src=b.d_dup_src[GUARD:], d_dup_first=b.d_dup_first[GUARD:])
    m, B = hb.ctx.uniq_compact_status()
    assert (m, B) == (len(exp[2]), len(exp[0]))
    v.accepted(exp[0], "uniq compact, 4 GiB below")
    u64 = lambda t, k: t.cpu().numpy().view(np.uint64)[GUARD:GUARD + k]
    UR.assert_equal((exp[0], u64(b.d_out_off, m + 1), u64(b.d_out_src, m), u64(b.d_dup_src, b.n - m), u64(b.d_dup_first, b.n - m)), exp, "uniq compact, 4 GiB below")
    b = Buffers(data, offs, fs)
    hb.ctx.uniq_compact_device(*args(hb.big[v.at_end:]), base_index=base, d_dup_src=b.d_dup_src[GUARD:], d_dup_first=b.d_dup_first[GUARD:])
    with pytest.raises(circkit_amd.CirckitError) as e:
        hb.ctx.uniq_compact_status()
    assert e.value.code == INVALID_ARG and "overlaps" in str(e.value)
    hb.unchanged("uniq compact, on the payload's last 16 bytes")
    for t, canary in ((b.d_out_src, SRC_CANARY), (b.d_dup_src, DSRC_CANARY), (b.d_dup_first, DFIRST_CANARY)):
        assert (t.cpu().numpy().view(np.uint64) == canary).all()


def _overlap_windows(hb, translate):
    import torch
    from tests import test_translate_gpu as TG
    from tests import test_windows_gpu as G
    from tests import translate_ref as T
    from tests import translate_sets as TS
    from tests import windows_ref as R
    from tests import windows_sets as S
    data, offs = (TS if translate else S).batch(np.random.default_rng(5))
    wins = R.windows_of_records(np.diff(offs.astype(np.int64)), R.CAT if translate else R.REVCOMP)
    code = TS.CODES[3]
    exp, exp_off, _ = T.windows_translate(data, offs, wins, *code) if translate else R.gather(data, offs, wins)
    total = len(exp)
    assert total >= 16
    v = Overlap(hb, data, offs)
    d_win = _to(wins.view(np.uint8))
    for out0, ok in ((v.below, True), (v.at_end, False)):
        d_out_off = canaried(len(wins) + 1, torch.int64, C64)
        if translate:
            hb.ctx.windows_translate_device(hb.big, v.d_offs, len(offs) - 1, d_win, len(wins), hb.big[out0:], total, d_out_off[GUARD:], params=TG.params(code))
            rc, got_total, bad = TG.status(hb.ctx)
        else:
            hb.ctx.windows_gather_device(hb.big, v.d_offs, len(offs) - 1, d_win, len(wins), hb.big[out0:], total, d_out_off[GUARD:])
            rc, got_total, bad = G.status(hb.ctx)
        assert (got_total, bad) == (total, 0) and np.array_equal(opened(d_out_off, len(wins) + 1, C64, np.uint64), exp_off)
        if ok:
            assert rc == OK
            v.accepted(exp, "4 GiB below")
        else:
            assert rc == INVALID_ARG and "overlaps" in hb.ctx._lib.circkit_last_error(hb.ctx._h).decode()
            hb.unchanged("on the payload's last 16 bytes")


def test_overlap_windows_gather(hb):
    _overlap_windows(hb, False)


def test_overlap_windows_translate(hb):
    _overlap_windows(hb, True)


def test_overlap_fasta_write_with_a_body(hb):
    import torch
    from tests import fasta_write_sets as S
    from tests import test_fasta_write_gpu as FW
    c = H.fasta_write_cases()[0]
    recs, bad = S.expected(c)
    want = b"".join(recs)
    data, offs = H.body_of(c)
    v = Overlap(hb, data, offs)
    assert bad == 0 and len(want) > len(data)
    text = FW.Image(c.text, 0)
    d_head = FW._to(c.head)
    for out0, ok in ((v.below, True), (v.at_end, False)):
        d_off = canaried(c.n_out + 1, torch.int64, C64)
        hb.ctx.fasta_write_device(text.d, len(c.text), d_head, len(c.head), c.n_out, hb.big[out0:], len(want), d_off[GUARD:], d_body=hb.big,
                                  d_body_offsets=v.d_offs)
        rc, total, n_bad, msg = FW.status(hb.ctx)
        assert (total, n_bad) == (len(want), 0) and text.unchanged()
        off = opened(d_off, c.n_out + 1, C64, np.uint64)
        assert np.array_equal(off, np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64))
        if ok:
            assert rc == OK, msg
            v.accepted(np.frombuffer(want, dtype=np.uint8), "FASTA write, 4 GiB below")
        else:
            assert rc == INVALID_ARG and "overlaps" in msg, msg
            hb.unchanged("FASTA write, on the body's last 16 bytes")
