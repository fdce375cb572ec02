"""GPU: circkit_fasta_parse_device / _status / _text against the host packer circkit_fasta_parse on the same text with the same
flags (tests/fasta_sets.py): the text sets of the CPU fiber test, and what only the device runs -- the scan over more than one
round of summaries, every pointer shift, capacities, refusals, back-to-back parses, streaming, the chain into canonicalize.
Record count, consumed, every offset, payload byte and span are compared; canaries surround the text and every output."""
import ctypes
import os

import numpy as np
import pytest

from tests import fasta_sets as S
from tests.emu import fasta_emu

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
WORD_CANARY = 0x25A5A5A5A5A5A5A5
OK, INVALID_ARG, OOM = 0, -1, -5
_C = fasta_emu.constants()
T = _C["TILE_BYTES"]
ROUND = _C["SCAN_WG"] * T                      # the text one round of the scan over the summaries covers


def _dev():
    import torch
    return torch.device("cuda", 0)


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
    """(rc, records, payload bytes, consumed, message) of the last parse, without raising."""
    r, b, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_fasta_parse_status(ctx._h, ctypes.byref(r), ctypes.byref(b), ctypes.byref(used))
    return rc, r.value, b.value, used.value, ctx._lib.circkit_last_error(ctx._h).decode() if rc else ""


class Buffers:
    """A text on the device at in_shift mod 16 and the four outputs (the payload at out_shift mod 16), canaries round each."""

    def __init__(self, text, record_room, byte_room, in_shift=0, out_shift=0, head=True, raw=True):
        import torch
        self.n, self.record_room, self.byte_room = len(text), record_room, byte_room
        img = np.full(GUARD + in_shift + self.n + GUARD, IN_CANARY, dtype=np.uint8)
        img[GUARD + in_shift:GUARD + in_shift + self.n] = np.frombuffer(bytes(text), dtype=np.uint8)
        self.img = img
        self.d_img = torch.from_numpy(img).to(_dev())
        self.d_text = self.d_img[GUARD + in_shift:]
        self.o0 = GUARD + out_shift
        self.d_raw_out = torch.full((self.o0 + byte_room + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        self.d_out = self.d_raw_out[self.o0:]
        self.d_off = torch.full((GUARD + record_room + 1 + GUARD,), WORD_CANARY, dtype=torch.int64, device=_dev())
        self.d_head = torch.full((GUARD + 2 * record_room + GUARD,), WORD_CANARY, dtype=torch.int64, device=_dev()) if head else None
        self.d_raw = torch.full((GUARD + 2 * record_room + GUARD,), WORD_CANARY, dtype=torch.int64, device=_dev()) if raw else None
        assert self.d_text.data_ptr() % 16 == in_shift % 16 and self.d_out.data_ptr() % 16 == out_shift % 16

    def launch(self, ctx, first, final, record_capacity=None, byte_capacity=None):
        ctx.fasta_parse_device(self.d_text, self.n, self.d_out, self.byte_room if byte_capacity is None else byte_capacity, self.d_off[GUARD:],
                               self.record_room if record_capacity is None else record_capacity,
                               self.d_head[GUARD:] if self.d_head is not None else None, self.d_raw[GUARD:] if self.d_raw is not None else None,
                               first_chunk=first, final_chunk=final)

    def result(self, records, nbytes, offsets_written=None):
        """dict(offsets, data, head, raw) after the canary checks; records / nbytes: what the parse may have written."""
        assert np.array_equal(self.d_img.cpu().numpy(), self.img), "the parse wrote into the text"
        out, off = self.d_raw_out.cpu().numpy(), _u64(self.d_off)
        assert (out[:self.o0] == OUT_CANARY).all() and (out[self.o0 + nbytes:] == OUT_CANARY).all(), "wrote outside [out, out + payload)"
        k = records + 1 if offsets_written is None else offsets_written
        assert (off[:GUARD] == WORD_CANARY).all() and (off[GUARD + k:] == WORD_CANARY).all(), "offsets written outside [0, records]"
        res = dict(offsets=off[GUARD:GUARD + k].copy(), data=out[self.o0:self.o0 + nbytes].copy(), head=None, raw=None)
        for name, t in (("head", self.d_head), ("raw", self.d_raw)):
            if t is not None:
                w = _u64(t)
                assert (w[:GUARD] == WORD_CANARY).all() and (w[GUARD + 2 * records:] == WORD_CANARY).all(), "%s spans written outside" % name
                res[name] = w[GUARD:GUARD + 2 * records].reshape(records, 2).copy()
        return res


def parse(ctx, text, first=True, final=True, what="", record_room=None, byte_room=None, **place):
    """Parses on the device into exactly sized buffers (the host's counts, unless rooms are given) and compares with the host."""
    exp = S.host(text, first, final)
    b = Buffers(text, exp["records"] if record_room is None else record_room, len(exp["data"]) if byte_room is None else byte_room, **place)
    b.launch(ctx, first, final)
    rc, records, nbytes, consumed, msg = status(ctx)
    if exp["error"]:
        assert (rc, records, nbytes, msg) == (INVALID_ARG, 0, 0, exp["error"]), (what, rc, records, nbytes, msg)
        res = b.result(0, 0)
        assert res["offsets"].tolist() == [0]
        return res
    assert rc == OK, (what, rc, msg)
    res = b.result(records, nbytes)
    res.update(refused=0, records=records, bytes=nbytes, consumed=consumed)
    S.same(res, exp, what=what)
    return res


# ---- 1. the text sets of the CPU fiber test ----------------------------------------------------------------------------------
SMALL, LARGE, EDGES = S.small_cases(), S.large_cases(), S.tile_edge_texts(T)


@pytest.mark.parametrize("pair", range(4), ids=["first_final", "first", "final", "middle"])
def test_small_texts(ctx, pair):
    first, final = S.FLAG_PAIRS[pair]
    for k, (name, t, f, l) in enumerate(SMALL):
        if (f, l) == (first, final):
            parse(ctx, t, f, l, what=name, in_shift=k % 16, out_shift=(5 * k + 3) % 16)


@pytest.mark.parametrize("pair", range(4), ids=["first_final", "first", "final", "middle"])
def test_large_texts(ctx, pair):
    first, final = S.FLAG_PAIRS[pair]
    for k, (name, t, f, l) in enumerate(LARGE):
        if (f, l) == (first, final):
            parse(ctx, t, f, l, what=name, in_shift=(3 * k) % 16, out_shift=(7 * k + 1) % 16)


def test_tile_edges(ctx):
    """Text lengths T - 1, T, T + 1, 2T - 1, 2T + 1; a record start as a tile's first and last byte ('\\n' the last byte of the
    tile before); a header of 2.5 tiles; a line of 3 tiles; tiles of dropped bytes only."""
    assert {len(t) for name, t, _, _ in EDGES if name.startswith("length")} == {T - 1, T, T + 1, 2 * T - 1, 2 * T + 1}
    for k, (name, t, f, l) in enumerate(EDGES):
        parse(ctx, t, f, l, what=name, in_shift=k % 16, out_shift=(k + 9) % 16)


# ---- 2. what only the device runs --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_text():
    """Wrapped records, a little over two rounds of the scan over the summaries."""
    return S.records_text(np.random.default_rng(31), (2 * ROUND + 3 * T) // 500 + 1, 500, width=70)


@pytest.mark.parametrize("tiles", [_C["SCAN_WG"] - 1, _C["SCAN_WG"], _C["SCAN_WG"] + 1, 2 * _C["SCAN_WG"] - 1, 2 * _C["SCAN_WG"], 2 * _C["SCAN_WG"] + 1])
def test_tile_count_round_a_round_of_the_scan(ctx, long_text, tiles):
    """One tile fewer than a round (and than two rounds) of the scan over the summaries, exactly a round, one more."""
    t = long_text[:tiles * T - 5]
    assert len(t) == tiles * T - 5
    parse(ctx, t, True, True, what=tiles)
    parse(ctx, t, True, False, what=tiles)


def test_every_shift_of_both_pointers(ctx, long_text):
    t = long_text[:3 * T + 123]
    for k in range(16):
        parse(ctx, t, True, k % 2 == 0, what=k, in_shift=k, out_shift=(5 * k + 3) % 16)
    assert {(5 * k + 3) % 16 for k in range(16)} == set(range(16))


def test_capacities_exact_and_one_less(ctx, long_text):
    t = long_text[:5 * T + 77]
    exp = S.host(t)
    R, B = exp["records"], len(exp["data"])
    for rec_cap, byte_cap, want in ((R, B, OK), (R - 1, B, OOM), (R, B - 1, OOM), (0, 0, OOM)):
        b = Buffers(t, R, B, in_shift=3, out_shift=11)
        b.launch(ctx, True, True, record_capacity=rec_cap, byte_capacity=byte_cap)
        rc, records, nbytes, consumed, msg = status(ctx)
        assert (rc, records, nbytes, consumed) == (want, R, B, len(t)), (rec_cap, byte_cap, rc, records, nbytes, msg)
        if want == OK:
            res = b.result(R, B)
            res.update(refused=0, records=records, bytes=nbytes, consumed=consumed)
            S.same(res, exp)
        else:
            assert str(R) in msg and str(B) in msg
            assert b.result(0, 0)["offsets"].tolist() == [0]          # nothing but offsets[0]: every other word is still canary
    # larger buffers than needed
    parse(ctx, t, record_room=(len(t) + 1) // 2, byte_room=len(t), out_shift=5)


@pytest.mark.parametrize("head,raw", [(False, False), (True, False), (False, True)])
def test_spans_not_asked_for(ctx, long_text, head, raw):
    res = parse(ctx, long_text[:2 * T + 9], head=head, raw=raw)
    assert (res["head"] is not None) == head and (res["raw"] is not None) == raw


def test_an_output_that_overlaps_the_text_is_refused(ctx, long_text):
    import torch
    t = long_text[:T + 300]
    exp = S.host(t)
    img = np.full(GUARD + 2 * len(t) + GUARD, IN_CANARY, dtype=np.uint8)
    img[GUARD:GUARD + len(t)] = np.frombuffer(t, dtype=np.uint8)
    d_img = torch.from_numpy(img).to(_dev())
    d_off = torch.full((exp["records"] + 1,), WORD_CANARY, dtype=torch.int64, device=_dev())
    for out_at, refused in ((GUARD + len(t) - 1, True), (GUARD + 7, True), (GUARD + len(t), False)):
        d_img.copy_(torch.from_numpy(img))
        ctx.fasta_parse_device(d_img[GUARD:], len(t), d_img[out_at:], len(t), d_off, exp["records"])
        rc, records, nbytes, consumed, msg = status(ctx)
        assert (records, nbytes, consumed) == (exp["records"], len(exp["data"]), len(t))
        got = d_img.cpu().numpy()
        if refused:
            assert rc == INVALID_ARG and "overlaps" in msg and np.array_equal(got, img)
        else:
            assert rc == OK and np.array_equal(got[out_at:out_at + nbytes], exp["data"]) and np.array_equal(got[:out_at], img[:out_at])


def test_two_parses_back_to_back(ctx, long_text):
    """Two parses enqueued one behind the other on one stream into different buffers, then one wait."""
    a, b = long_text[:3 * T + 1], long_text[T // 2 + 11:T // 2 + 11 + 2 * T]
    ea, eb = S.host(a), S.host(b, False, False)
    ba = Buffers(a, ea["records"], len(ea["data"]), out_shift=1)
    bb = Buffers(b, eb["records"], len(eb["data"]), in_shift=9, out_shift=6)
    ba.launch(ctx, True, True)
    bb.launch(ctx, False, False)
    rc, records, nbytes, consumed, msg = status(ctx)
    assert (rc, records, nbytes, consumed) == (OK, eb["records"], len(eb["data"]), eb["consumed"])        # the most recent parse's
    for buf, exp in ((ba, ea), (bb, eb)):
        res = buf.result(exp["records"], len(exp["data"]))
        res.update(refused=0, records=exp["records"], bytes=len(exp["data"]), consumed=exp["consumed"])
        S.same(res, exp)


def test_streaming_in_eight_chunks(ctx):
    """A text of about 1 MB cut at 7 arbitrary points: every chunk is parsed behind the remainder of the one before, and the
    batches in a row are the one-shot host parse."""
    rng = np.random.default_rng(77)
    text = S.records_text(rng, 1500, 620, width=80, crlf=True)[:-2]          # (the last line unterminated)
    whole = S.host(text)
    cuts = [0] + sorted(int(c) for c in rng.integers(1, len(text), size=7)) + [len(text)]
    data, offsets, head, raw = [], [np.zeros(1, dtype=np.uint64)], [], []
    rest, at = b"", 0                                                        # `rest` begins at position `at` of the text
    for k in range(8):
        buf = rest + text[cuts[k]:cuts[k + 1]]
        res = parse(ctx, buf, k == 0, k == 7, what=k, in_shift=k, out_shift=15 - k)
        data.append(res["data"])
        offsets.append(res["offsets"][1:] + offsets[-1][-1])
        for spans, into in ((res["head"], head), (res["raw"], raw)):
            spans[:, 0] += np.uint64(at)
            into.append(spans)
        rest, at = buf[res["consumed"]:], at + res["consumed"]
    assert rest == b"" and at == len(text)
    got = dict(refused=0, records=sum(len(h) for h in head), consumed=at, bytes=sum(len(d) for d in data), data=np.concatenate(data),
               offsets=np.concatenate(offsets), head=np.concatenate(head), raw=np.concatenate(raw))
    S.same(got, whole)


# ---- 3. the host form and the Python surface ---------------------------------------------------------------------------------
def test_parse_text_is_fasta_parse(ctx):
    import circkit_amd
    from circkit_amd import api
    texts = [t for _, t in S.golden_texts()] + [t for t, _, _ in S.TABLE] + S.CORNERS[:8] + [S.records_text(np.random.default_rng(3), 40, 700, width=60)]
    for t in texts:
        for first, final in S.FLAG_PAIRS:
            if not S.deterministic(t, first, final):
                continue
            try:
                exp = api.fasta_parse(t, first, final)
            except ValueError as e:
                with pytest.raises(ValueError, match="expected '>'"):
                    ctx.fasta_parse_text(t, first, final)
                assert str(e) == S.FORMAT_ERROR
                continue
            got = ctx.fasta_parse_text(t, first, final)
            assert got[0] == exp[0] and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]) and got[3] == exp[3], (t[:40], first, final)
    t = texts[-1]
    exp, got = api.fasta_parse(t), circkit_amd.fasta_parse_gpu(t)
    assert got[0] == exp[0] and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2]) and got[3] == exp[3]


def test_parse_text_with_small_buffers(ctx):
    """circkit_fasta_parse_text: OOM with the true counts and nothing but out_offsets[0] written, then the call again."""
    t = S.records_text(np.random.default_rng(4), 12, 300, width=50)
    exp = S.host(t)
    R, B = exp["records"], len(exp["data"])
    buf = np.frombuffer(t, dtype=np.uint8)
    for rec_cap, byte_cap, want in ((R, B - 1, OOM), (R - 1, B, OOM), (R, B, OK)):
        data = np.full(B + 8, OUT_CANARY, dtype=np.uint8)
        offs = np.full(R + 1 + 8, WORD_CANARY, dtype=np.uint64)
        head, raw = np.full((R + 4, 2), WORD_CANARY, dtype=np.uint64), np.full((R + 4, 2), WORD_CANARY, dtype=np.uint64)
        r, b, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = ctx._lib.circkit_fasta_parse_text(ctx._h, buf.ctypes.data, len(t), 1, 1, data.ctypes.data, byte_cap, offs.ctypes.data, rec_cap,
                                               head.ctypes.data, raw.ctypes.data, ctypes.byref(r), ctypes.byref(b), ctypes.byref(used))
        assert (rc, r.value, b.value, used.value) == (want, R, B, len(t))
        if want == OK:
            got = dict(refused=0, records=R, bytes=B, consumed=used.value, offsets=offs[:R + 1], data=data[:B], head=head[:R], raw=raw[:R])
            S.same(got, exp)
            assert (data[B:] == OUT_CANARY).all() and (offs[R + 1:] == WORD_CANARY).all() and (head[R:] == WORD_CANARY).all() and (raw[R:] == WORD_CANARY).all()
        else:
            assert offs[0] == 0 and (offs[1:] == WORD_CANARY).all() and (data == OUT_CANARY).all() and (head == WORD_CANARY).all()


def test_chain_text_to_canonical(ctx):
    """fasta_parse_text(keep_on_device=True) -> canonicalize_batch_device equals canonicalize_batch(fasta_parse(text))."""
    import torch
    from circkit_amd import api
    text = open(os.path.join(S.GOLDEN, "nim_cated", "realistic_input.fasta"), "rb").read()
    recs, data, offs, consumed = api.fasta_parse(text)
    exp = ctx.canonicalize_batch(data, offs)["bytes"]
    d_recs, d_data, d_offs, d_consumed = ctx.fasta_parse_text(text, keep_on_device=True)
    assert d_recs == recs and d_consumed == consumed and len(d_offs) == len(offs) and len(d_data) == len(data) and len(recs) > 0
    assert np.array_equal(_u64(d_offs), offs) and np.array_equal(d_data.cpu().numpy(), data)
    d_out = torch.full((len(data) + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.canonicalize_batch_device(d_data, d_offs, len(recs), out_bytes=d_out)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[:len(data)], exp) and (out[len(data):] == OUT_CANARY).all()
