"""GPU: circkit_fasta_write_device / _status / _text.  Per record the yardstick is the Python join b">" + head + label + b"\\n" +
body + b"\\n" (tests/fasta_write_sets.py: the case sets of the CPU fiber test); for whole files the pinned writers of canonicalize,
uniq, rotate, cat, decat and orfs on the reference's own fixtures, with text on the device from the parse to the written text.
What only the device runs: the scan over more than one round of tile sums, back-to-back writes, the totals next to a gather's,
the host form.  Canaries surround the text, the body and every output; refused and invalid inputs are checked by status and
canaries."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as O
from tests import fasta_write_sets as S
from tests import orfs_ref
from tests.emu import fasta_write_emu

pytestmark = pytest.mark.gpu

GUARD = 64
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
WORD_CANARY = 0x25A5A5A5A5A5A5A5
OK, INVALID_ARG, OOM = 0, -1, -5
_C = fasta_write_emu.constants()
T, SCAN_TILE, SCAN_WG = _C["TILE_BYTES"], _C["SCAN_TILE"], _C["SCAN_WG"]
ROTATE_FLAGS = {"rotate_5": dict(bases=5), "rotate_minus_5": dict(bases=-5), "rotate_0.25": dict(percent=0.25), "rotate_0.5": dict(percent=0.5)}
GOLDEN = S.golden_inputs()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    """A numpy array on the device (8-byte words as int64, anything else as bytes)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize == 8 and a.dtype.kind in "ui":
        return torch.from_numpy(a.view(np.int64).reshape(-1).copy()).to(_dev()) if a.size else torch.zeros(1, dtype=torch.int64, device=_dev())
    b = np.frombuffer(a.tobytes(), dtype=np.uint8)
    return torch.from_numpy(b.copy()).to(_dev()) if b.size else torch.zeros(8, dtype=torch.uint8, device=_dev())


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _words(n):
    import torch
    return torch.empty(max(n, 1), dtype=torch.int64, device=_dev())


def _bytes(n):
    import torch
    return torch.empty(max(n, 1) + 64, dtype=torch.uint8, device=_dev())


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
    """(rc, total, invalid records, message) of the last write, without raising."""
    t, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_fasta_write_status(ctx._h, ctypes.byref(t), ctypes.byref(bad))
    return rc, t.value, bad.value, ctx._lib.circkit_last_error(ctx._h).decode() if rc else ""


class Image:
    """Bytes on the device at `shift` mod 16 with `room` canary bytes on either side (an output may be placed there)."""

    def __init__(self, data, shift, room=0):
        import torch
        data = np.frombuffer(bytes(data), dtype=np.uint8)
        self.at = GUARD + shift + room
        img = np.full(self.at + len(data) + room + GUARD, IN_CANARY, dtype=np.uint8)
        img[self.at:self.at + len(data)] = data
        self.img = img
        self.d_img = torch.from_numpy(img).to(_dev())
        self.d = self.d_img[self.at:]
        assert self.d.data_ptr() % 16 == (shift + room) % 16

    def unchanged(self, lo=0, hi=0):
        """Everything but the image's bytes [lo, hi) (positions in the whole image) is as it was."""
        now = self.d_img.cpu().numpy()
        return np.array_equal(now[:lo], self.img[:lo]) and np.array_equal(now[hi:], self.img[hi:]) if hi > lo else np.array_equal(now, self.img)


class Run:
    """One case on the device: its buffers, the launch, and the result after the canary checks."""

    def __init__(self, c, total):
        import torch
        p = c.place
        self.c, self.alias, self.total = c, p.get("alias", 0), total
        self.capacity = total if p.get("capacity", S.EXACT) == S.EXACT else p["capacity"]
        room = total + 48 if self.alias else 0
        self.text = Image(c.text, p.get("text_shift", 0), room if self.alias == S.ALIAS_TEXT else 0)
        self.body = Image(c.body.tobytes(), p.get("body_shift", 0), room if self.alias == S.ALIAS_BODY else 0) if c.body is not None else None
        self.d_head, self.d_raw = _to(c.head), _to(c.raw) if c.raw is not None else None
        self.d_src = _to(c.src) if c.src is not None else None
        self.d_labels = _to(c.labels) if c.labels is not None else None
        self.d_body_off = _to(c.offsets) if c.offsets is not None else None
        self.o0 = GUARD + p.get("out_shift", 0)
        self.d_out_img = torch.full((self.o0 + (0 if self.alias else self.capacity) + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        if self.alias == S.ALIAS_TEXT:
            self.host, self.out_at = self.text, self.text.at + p["alias_at"]
        elif self.alias == S.ALIAS_BODY:
            self.host, self.out_at = self.body, self.body.at + int(c.offsets[0]) + p["alias_at"]
        else:
            self.host, self.out_at = None, self.o0
        self.d_out = (self.host.d_img if self.host else self.d_out_img)[self.out_at:]
        self.d_off = torch.full((GUARD + c.n_out + 1 + GUARD,), WORD_CANARY, dtype=torch.int64, device=_dev())

    def launch(self, ctx):
        c = self.c
        ctx.fasta_write_device(self.text.d, len(c.text), self.d_head, len(c.head), c.n_out, self.d_out, self.capacity, self.d_off[GUARD:],
                               d_body=self.body.d if self.body else None, d_body_offsets=self.d_body_off, d_raw=self.d_raw, d_src=self.d_src,
                               n_src=c.n_src, d_labels=self.d_labels)

    def result(self, written):
        """(text | None, offsets): the first `written` output bytes (None when the write was refused: every output byte is still
        canary then) after checking that nothing else changed."""
        lo, hi = self.out_at, self.out_at + written
        for img in (self.text, self.body):
            if img is not None:
                assert img.unchanged(lo, hi) if img is self.host else img.unchanged(), "the write changed an input"
        out = self.d_out_img.cpu().numpy()
        if self.host is None:
            assert (out[:lo] == OUT_CANARY).all() and (out[hi:] == OUT_CANARY).all(), "wrote outside [out, out + total)"
        else:
            assert (out == OUT_CANARY).all()
        off = _u64(self.d_off)
        assert (off[:GUARD] == WORD_CANARY).all() and (off[GUARD + self.c.n_out + 1:] == WORD_CANARY).all(), "offsets written outside [0, n_out]"
        src = self.host.d_img if self.host else self.d_out_img
        return (src[lo:hi].cpu().numpy().tobytes() if written or not self.refused else None), off[GUARD:GUARD + self.c.n_out + 1].copy()

    refused = 0


def run_case(ctx, c, accepted=True):
    """The case through the device; an accepted one is compared with the join, a refused one returns (rc, total, message, offsets)."""
    recs, bad = S.expected(c)
    total = 2 ** 64 - 1 if c.name == "total_beyond_64_bits" else sum(len(r) for r in recs)
    r = Run(c, total if accepted else 0 if c.name == "total_beyond_64_bits" else total)
    r.launch(ctx)
    rc, got_total, got_bad, msg = status(ctx)
    if accepted:
        assert rc == (INVALID_ARG if bad else OK) and (not bad or "%d invalid records" % bad in msg), (c.name, rc, msg)
        text, off = r.result(got_total)
        S.check(c, (text or b"", off, got_total, got_bad, 0))
        return None
    r.refused = 1
    assert got_total == total, (c.name, got_total, total)
    text, off = r.result(0)
    assert text is None
    return rc, got_total, msg, off


# ---- 1. the case sets of the CPU fiber test ----------------------------------------------------------------------------------
SETS = {"grid": S.grid_cases, "long_and_seams": lambda: S.long_cases(T) + S.seam_cases(T), "labels_maps_raw": lambda: S.label_cases() + S.map_cases() +
        S.raw_cases(), "invalid": S.invalid_cases}


@pytest.mark.parametrize("name", sorted(SETS))
def test_the_sets_on_the_card(ctx, name):
    cases = SETS[name]()
    assert len(cases) >= 2
    for c in cases:
        run_case(ctx, c)


def test_capacity(ctx):
    """Exact, one less, 0, more; no records; a total beyond 64 bits.  After a refusal every output byte is still canary, the
    offsets are written in full and no word beyond them is."""
    for c, ok in S.capacity_cases():
        if ok:
            run_case(ctx, c)
            continue
        rc, total, msg, off = run_case(ctx, c, accepted=False)
        assert rc == OOM and str(total) in msg and "nothing was written" in msg, (c.name, rc, msg)
        if c.name != "total_beyond_64_bits":
            assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in S.expected(c)[0]])]).tolist()
        else:
            assert off[0] == 0 and off[-1] == 2 ** 64 - 1


def test_overlap(ctx):
    for c, ok in S.overlap_cases():
        if ok:
            run_case(ctx, c)
        else:
            rc, total, msg, off = run_case(ctx, c, accepted=False)
            assert rc == INVALID_ARG and "overlaps" in msg, (c.name, rc, msg)
            assert int(off[-1]) == total


def test_argument_errors(ctx):
    """Null / non-null combinations that make no sense: INVALID_ARG, nothing enqueued, nothing written."""
    import circkit_amd
    c = S.raw_cases()[0]
    r = Run(c, sum(len(x) for x in S.expected(c)[0]))
    good = dict(d_text=r.text.d, n_text=len(c.text), d_head=r.d_head, n_heads=len(c.head), n_out=c.n_out, d_out_text=r.d_out, out_capacity=r.capacity,
                d_out_offsets=r.d_off[GUARD:], d_raw=r.d_raw)
    body = _to(np.zeros(16, dtype=np.uint8))
    for change in (dict(d_raw=None), dict(d_body=body, d_body_offsets=_to(np.zeros(c.n_out + 1, dtype=np.uint64))), dict(d_raw=None, d_body=body),
                   dict(d_out_offsets=None), dict(d_out_text=None), dict(d_head=None), dict(d_text=None), dict(n_src=c.n_out + 1), dict(n_text=2 ** 40 + 1)):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.fasta_write_device(**dict(good, **change))
        assert e.value.code == INVALID_ARG, change
    text, off = r.result(0)
    assert (off == WORD_CANARY).all()
    assert ctx._lib.circkit_fasta_write_device(None, None, 0, None, None, 0, None, 0, None, None, None, 0, None, 0, None) == INVALID_ARG and ctx._lib.circkit_fasta_write_status(None, None, None) == INVALID_ARG
    ctx.fasta_write_device(**good)                                              # the next valid call works
    assert status(ctx)[:3] == (OK, r.total, 0)
    S.check(c, (r.result(r.total)[0], r.result(r.total)[1], r.total, 0, 0))


# ---- 2. what only the device runs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", [SCAN_WG - 1, SCAN_WG, SCAN_WG + 1])
def test_tile_count_round_a_round_of_the_scan(ctx, tiles):
    """One tile of the scan fewer than a round of its middle kernel, exactly a round, one more: records of 3 bytes, and of 40."""
    import torch
    m = tiles * SCAN_TILE - 7
    assert (m + SCAN_TILE - 1) // SCAN_TILE == tiles
    rng = np.random.default_rng(tiles)
    heads = rng.integers(ord("a"), ord("z") + 1, size=(m, 5), dtype=np.uint8)
    bodies = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(m, 32))]
    want40 = np.concatenate([np.full((m, 1), ord(">"), np.uint8), heads, np.full((m, 1), 10, np.uint8), bodies, np.full((m, 1), 10, np.uint8)], axis=1)
    spans = np.stack([5 * np.arange(m, dtype=np.uint64), np.full(m, 5, dtype=np.uint64)], axis=1)
    d_text, d_body = _to(heads), _to(bodies)
    d_body_off = _to(32 * np.arange(m + 1, dtype=np.uint64))
    for spans_k, body_off, want in ((spans, d_body_off, want40.reshape(-1)), (np.zeros((m, 2), dtype=np.uint64), _to(np.zeros(m + 1, dtype=np.uint64)),
                                                                             np.tile(np.frombuffer(b">\n\n", dtype=np.uint8), m))):
        d_out = torch.full((GUARD + 3 + len(want) + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
        d_off = torch.full((m + 1 + GUARD,), WORD_CANARY, dtype=torch.int64, device=_dev())
        ctx.fasta_write_device(d_text, 5 * m, _to(spans_k), m, m, d_out[GUARD + 3:], len(want), d_off, d_body=d_body, d_body_offsets=body_off)
        assert status(ctx) == (OK, len(want), 0, "")
        out, off = d_out.cpu().numpy(), _u64(d_off)
        assert np.array_equal(out[GUARD + 3:GUARD + 3 + len(want)], want)
        assert (out[:GUARD + 3] == OUT_CANARY).all() and (out[GUARD + 3 + len(want):] == OUT_CANARY).all() and (off[m + 1:] == WORD_CANARY).all()
        assert np.array_equal(off[:m + 1], (len(want) // m) * np.arange(m + 1, dtype=np.uint64))


def test_two_writes_back_to_back(ctx):
    """Two writes enqueued one behind the other on one stream into different buffers, then one wait."""
    a, b = S.grid_cases()[2], S.label_cases()[0]
    runs = [Run(c, sum(len(x) for x in S.expected(c)[0])) for c in (a, b)]
    for r in runs:
        r.launch(ctx)
    assert status(ctx)[:3] == (OK, runs[1].total, 0)                            # the most recent write's
    for c, r in zip((a, b), runs):
        text, off = r.result(r.total)
        S.check(c, (text, off, r.total, 0, 0))


def test_the_totals_are_the_writes_own(ctx):
    """A write between a gather and its circkit_windows_status, and between a parse and its status: each answers for its kind."""
    import torch
    from circkit_amd import api
    text = GOLDEN["cat"]
    P = parse_on_device(ctx, text)
    R, B = P["R"], P["B"]
    d_win = torch.empty(R * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
    ctx.windows_of_records_device(P["d_off"], R, "cat", d_win)
    d_wout, d_woff = _bytes(2 * B), _words(R + 1)
    ctx.windows_gather_device(P["d_data"], P["d_off"], R, d_win, R, d_wout, 2 * B, d_woff)
    c = S.invalid_cases()[0]
    recs, bad = S.expected(c)
    r = Run(c, sum(len(x) for x in recs))
    r.launch(ctx)
    assert ctx.windows_status() == (2 * B, 0) and ctx.fasta_parse_status()[:2] == (R, B)
    rc, total, got_bad, msg = status(ctx)
    assert (rc, total, got_bad) == (INVALID_ARG, r.total, bad) and bad > 0 and 2 * B != r.total
    assert ctx.windows_status() == (2 * B, 0)                                   # and again, after the other status call
    S.check(c, r.result(r.total) + (total, got_bad, 0))


def test_write_text_is_the_join(ctx):
    import circkit_amd
    cases = S.label_cases() + S.map_cases()[:4] + S.raw_cases() + [S.grid_cases()[1], S.long_cases(T)[0]]
    for c in cases:
        assert not c.place.get("alias") and S.expected(c)[1] == 0
        text, off = ctx.fasta_write_text(c.text, c.head, body=c.body, offsets=c.offsets, raw=c.raw, src=c.src, labels=c.labels)
        assert isinstance(text, bytes)
        S.check(c, (text, off, len(text), 0, 0))
    c = cases[0]
    text, off = circkit_amd.fasta_write_gpu(c.text, c.head, body=c.body, offsets=c.offsets, labels=c.labels)
    S.check(c, (text, off, len(text), 0, 0))
    bad = S.invalid_cases()[0]
    with pytest.raises(circkit_amd.CirckitError, match="invalid records"):
        ctx.fasta_write_text(bad.text, bad.head, body=bad.body, offsets=bad.offsets, labels=bad.labels)


def test_write_text_with_a_buffer_one_short(ctx):
    """circkit_fasta_write_text: OOM with the total returned, the offsets written and no byte of text; then the call again."""
    c = S.map_cases()[2]
    want = b"".join(S.expected(c)[0])
    buf = np.frombuffer(c.text, dtype=np.uint8)
    for cap, rc_want in ((len(want) - 1, OOM), (0, OOM), (len(want), OK)):
        out = np.full(len(want) + 8, OUT_CANARY, dtype=np.uint8)
        off = np.full(c.n_out + 1 + 4, WORD_CANARY, dtype=np.uint64)
        total = ctypes.c_uint64(0)
        rc = ctx._lib.circkit_fasta_write_text(ctx._h, buf.ctypes.data, len(c.text), c.head.ctypes.data, None, len(c.head), c.src.ctypes.data, c.n_src,
                                               None, c.body.ctypes.data, c.offsets.ctypes.data, c.n_out, out.ctypes.data, cap, off.ctypes.data,
                                               ctypes.byref(total))
        assert (rc, total.value) == (rc_want, len(want)) and int(off[c.n_out]) == len(want) and (off[c.n_out + 1:] == WORD_CANARY).all()
        assert status(ctx)[:2] == (rc_want, len(want))
        if rc_want == OK:
            assert out[:len(want)].tobytes() == want and (out[len(want):] == OUT_CANARY).all()
        else:
            assert (out == OUT_CANARY).all()


# ---- 3. text to text ---------------------------------------------------------------------------------------------------------
def parse_on_device(ctx, text):
    """circkit_fasta_parse_device with spans: the text, the batch and the spans stay on the device."""
    n = len(text)
    cap = (n + 1) // 2
    P = dict(d_text=_to(np.frombuffer(text, dtype=np.uint8)), n=n, d_data=_bytes(n), d_off=_words(cap + 1), d_head=_words(2 * cap), d_raw=_words(2 * cap))
    ctx.fasta_parse_device(P["d_text"], n, P["d_data"], n, P["d_off"], cap, P["d_head"], P["d_raw"])
    P["R"], P["B"], used = ctx.fasta_parse_status()
    assert used == n
    return P


def write_on_device(ctx, P, n_out, **kw):
    """The written text: a write without room for the total (OOM), then one into a buffer of exactly that size between canaries."""
    import torch
    d_off = _words(n_out + 1)
    ctx.fasta_write_device(P["d_text"], P["n"], P["d_head"], P["R"], n_out, None, 0, d_off, **kw)
    rc, total, bad, msg = status(ctx)
    assert bad == 0 and rc == (OOM if total else OK), (rc, msg)
    d_out = torch.full((GUARD + 5 + total + GUARD,), OUT_CANARY, dtype=torch.uint8, device=_dev())
    ctx.fasta_write_device(P["d_text"], P["n"], P["d_head"], P["R"], n_out, d_out[GUARD + 5:], total, d_off, **kw)
    assert status(ctx) == (OK, total, 0, "")
    out = d_out.cpu().numpy()
    assert (out[:GUARD + 5] == OUT_CANARY).all() and (out[GUARD + 5 + total:] == OUT_CANARY).all()
    assert int(_u64(d_off)[n_out]) == total
    return out[GUARD + 5:GUARD + 5 + total].tobytes()


def canonical_on_device(ctx, d_data, d_off, n):
    d_canon, d_hash = _bytes(int(_u64(d_off)[n]) if n else 0), _words(n)
    if n:
        ctx.canonicalize_batch_device(d_data, d_off, n, out_bytes=d_canon, out_xxh3=d_hash)
    return d_canon, d_hash


def uniq_on_device(ctx, d_canon, d_off, d_hash, n):
    """(kept records, d_bytes, d_offsets, d_out_src) of the uniq compact behind the table's resolve."""
    d_fs, d_ub, d_uoff, d_usrc = _words(n), _bytes(int(_u64(d_off)[n]) if n else 0), _words(n + 1), _words(n)
    if not n:
        return 0, d_ub, d_uoff.zero_(), d_usrc
    ctx.uniq_reset(n)
    ctx.uniq_resolve_device(d_hash, n, 0, d_fs)
    ctx.uniq_compact_device(d_canon, d_off, n, d_fs, d_ub, d_uoff, d_usrc)
    m, _ = ctx.uniq_compact_status()
    return m, d_ub, d_uoff, d_usrc


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_chain_text_to_text(ctx, name):
    """Text on the device, circkit_fasta_parse_device with spans, a command's kernels, circkit_fasta_write_device: the written
    text is the pinned writer's file."""
    import torch
    from circkit_amd import api
    text = GOLDEN[name]
    P = parse_on_device(ctx, text)
    R, B = P["R"], P["B"]
    assert R == len(O.read_fasta(text)) and R > 0
    d_canon, d_hash = canonical_on_device(ctx, P["d_data"], P["d_off"], R)
    assert write_on_device(ctx, P, R, d_body=d_canon, d_body_offsets=P["d_off"]) == O.cli_canonicalize(text)
    m, d_ub, d_uoff, d_usrc = uniq_on_device(ctx, d_canon, P["d_off"], d_hash, R)
    assert write_on_device(ctx, P, m, d_body=d_ub, d_body_offsets=d_uoff, d_src=d_usrc, n_src=m) == O.cli_uniq(text, True)[0]
    assert write_on_device(ctx, P, m, d_raw=P["d_raw"], d_src=d_usrc, n_src=m) == O.cli_uniq(text, False)[0]
    if name in S.NOT_FOR_WINDOWS:
        return
    runs = [("cat", {}, O.cli_cat(text)), ("decat", {}, O.cli_decat(text))]
    if name in ROTATE_FLAGS:
        flags = ROTATE_FLAGS[name]
        runs.append(("rotate_bases" if "bases" in flags else "rotate_percent", flags, O.cli_rotate(text, **flags)))
    d_win = torch.empty(R * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
    d_wout, d_woff = _bytes(2 * B), _words(R + 1)
    for kind, kw, want in runs:
        ctx.windows_of_records_device(P["d_off"], R, kind, d_win, **kw)
        ctx.windows_gather_device(P["d_data"], P["d_off"], R, d_win, R, d_wout, 2 * B, d_woff)
        ctx.windows_status()
        assert write_on_device(ctx, P, R, d_body=d_wout, d_body_offsets=d_woff) == want, (name, kind)


def test_chain_orfs_and_proteins(ctx):
    """orfs -> orfs windows -> gather -> write with the windows as labels is `circkit orfs`'s file; translate -> write with the
    same labels is the join of the same ids and the proteins."""
    import torch
    from circkit_amd import api
    text = GOLDEN["realistic_input"]
    P = parse_on_device(ctx, text)
    R, B = P["R"], P["B"]
    p = api.orf_params(min_length=75, max_wraps=3, require_stop=True)
    d_orf_off, cap = _words(R + 1), 4 * R
    while True:
        d_orfs = torch.empty(cap * api.ORF_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
        ctx.orfs_batch_device(P["d_data"], P["d_off"], R, d_orf_off, d_orfs, cap, params=p)
        t = ctypes.c_uint64(0)
        rc = ctx._lib.circkit_orfs_status(ctx._h, ctypes.byref(t))
        if rc == OOM and t.value > cap:
            cap = t.value
            continue
        assert rc == OK
        break
    n_orfs = t.value
    assert n_orfs > 100
    d_win = torch.empty(n_orfs * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=_dev())
    ctx.orfs_windows_device(d_orf_off, d_orfs, R, n_orfs, d_win)
    lengths = d_win.cpu().numpy().view(api.WINDOW_DTYPE)["length"]
    total = int(lengths.sum())
    d_seq, d_seq_off = _bytes(total), _words(n_orfs + 1)
    ctx.windows_gather_device(P["d_data"], P["d_off"], R, d_win, n_orfs, d_seq, total, d_seq_off)
    assert ctx.windows_status() == (total, 0)
    got = write_on_device(ctx, P, n_orfs, d_body=d_seq, d_body_offsets=d_seq_off, d_labels=d_win)
    assert got == orfs_ref.cli_orfs(text)[0]
    d_aa, d_aa_off = _bytes(total // 3), _words(n_orfs + 1)
    ctx.windows_translate_device(P["d_data"], P["d_off"], R, d_win, n_orfs, d_aa, total // 3, d_aa_off)
    n_aa, _ = ctx.translate_status()
    got = write_on_device(ctx, P, n_orfs, d_body=d_aa, d_body_offsets=d_aa_off, d_labels=d_win)
    heads = [h for h, _ in O.read_fasta(text)]
    wins, aa, aa_off = d_win.cpu().numpy().view(api.WINDOW_DTYPE), d_aa.cpu().numpy(), _u64(d_aa_off)
    want = b"".join(b">" + heads[int(w["record"])] + S.label_of(int(w["strand"]), int(w["start"])) + b"\n" + aa[int(a):int(b)].tobytes() + b"\n"
                    for w, a, b in zip(wins, aa_off[:-1], aa_off[1:]))
    assert got == want and n_aa == int(aa_off[n_orfs]) > 0


def test_chain_through_both_compacts(ctx):
    """monomerize compact -> canonicalize -> uniq compact: the two kept-record maps composed by a torch index name the headers."""
    import torch
    text = GOLDEN["realistic_input"]
    P = parse_on_device(ctx, text)
    R, B = P["R"], P["B"]
    d_end = torch.empty(R, dtype=torch.int32, device=_dev())
    ctx.monomerize_batch_device(P["d_data"], P["d_off"], R, d_end)
    d_mono, d_moff, d_msrc = _bytes(B), _words(R + 1), _words(R)
    ctx.monomers_compact_device(P["d_data"], P["d_off"], R, d_end, d_mono, d_moff, d_msrc)
    m1, _ = ctx.monomers_status()
    d_canon, d_hash = canonical_on_device(ctx, d_mono, d_moff, m1)
    m2, d_ub, d_uoff, d_usrc = uniq_on_device(ctx, d_canon, d_moff, d_hash, m1)
    assert 0 < m2 <= m1 <= R
    d_map = d_msrc[d_usrc[:m2]].contiguous()
    got = write_on_device(ctx, P, m2, d_body=d_ub, d_body_offsets=d_uoff, d_src=d_map, n_src=m2)
    heads = [h for h, _ in O.read_fasta(text)]
    msrc, usrc, ub, uoff = _u64(d_msrc), _u64(d_usrc), d_ub.cpu().numpy(), _u64(d_uoff)
    want = b"".join(b">" + heads[int(msrc[int(usrc[j])])] + b"\n" + ub[int(uoff[j]):int(uoff[j + 1])].tobytes() + b"\n" for j in range(m2))
    assert got == want and len(set(int(msrc[int(u)]) for u in usrc[:m2])) == m2
