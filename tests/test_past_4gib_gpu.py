"""GPU: text and outputs that are themselves longer than 4 GiB (run with -m gpu).

tests/test_high_base_gpu.py puts small sets at a high base; here the FASTA text, the kept bytes of both compacts, the bytes of the
windows gather and the residues of the translate each pass 2^32, so that an output position, a text position or a span offset
truncated to 32 bits shows.  All generation and all comparison happen on the device (torch, circkit_synth_fill_device); what
the host contributes is the yardstick's answer for one block or one period, a few kB, and the arithmetic that tiles it.  Every
comparison is exact; no test holds more than about 16 GiB, and each frees its tensors before the next."""
import numpy as np
import pytest

from tests import high_base as H

pytestmark = pytest.mark.gpu

LINE = H.LINE
MIB = 1 << 20


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


@pytest.fixture
def ctx():
    """A ctx on torch's stream; the tensors of the test are gone and the cache is empty before the next test begins."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def rows_equal(d_rows, d_row, chunk=1 << 20):
    """Every row of the (R, P) view equals the one row, compared on the device in chunks of rows (no 4 GiB temporary)."""
    for a in range(0, d_rows.shape[0], chunk):
        if not bool((d_rows[a:a + chunk] == d_row).all()):
            return False
    return True


# ---- B1 / B2: FASTA text beyond 2^32 ---------------------------------------------------------------------------------------------
class Parsed:
    """A tiled text on the device, parsed there, and checked against the arithmetic on the host parse of one block."""

    def __init__(self, ctx, where, byte_capacity=None, repeats=0):
        import torch
        from tests import fasta_sets as F
        self.block = block = H.block_for(where)
        self.one = one = F.host(block)
        self.Lb, self.r, self.P = len(block), one["records"], len(one["data"])
        self.R = R = max(-(-(LINE + 64 * MIB) // self.Lb), repeats)
        self.n_text, self.n_rec = R * self.Lb, R * self.r
        assert self.n_text > LINE + 64 * MIB and H.where_line_falls(block) == where
        self.d_text = _to(np.frombuffer(block, dtype=np.uint8)).repeat(R)
        self.capacity = self.n_text if byte_capacity is None else byte_capacity(self)
        self.d_out = torch.empty(self.capacity, dtype=torch.uint8, device=_dev())
        self.d_off = torch.full((self.n_rec + 1,), -1, dtype=torch.int64, device=_dev())
        self.d_spans = torch.full((2, self.n_rec, 2), -1, dtype=torch.int64, device=_dev())
        ctx.fasta_parse_device(self.d_text, self.n_text, self.d_out, self.capacity, self.d_off, self.n_rec, self.d_spans[0], self.d_spans[1])
        self.status = ctx.fasta_parse_status()

    def check(self):
        import torch
        R, r, P, Lb, one = self.R, self.r, self.P, self.Lb, self.one
        assert self.status == (R * r, R * P, self.n_text), self.status
        i = torch.arange(R, dtype=torch.int64, device=_dev())[:, None]
        assert torch.equal(self.d_off[:R * r].view(R, r), i * P + _to(_i64(one["offsets"][:r]))[None, :]) and int(self.d_off[R * r]) == R * P
        assert rows_equal(self.d_out[:R * P].view(R, P), _to(one["data"])), "the payload is not the block's payload tiled"
        for k, key in enumerate(("head", "raw")):
            s = self.d_spans[k].view(R, r, 2)
            assert torch.equal(s[:, :, 0], i * Lb + _to(_i64(one[key][:, 0]))[None, :]), key
            assert torch.equal(s[:, :, 1], _to(_i64(one[key][:, 1]))[None, :].expand(R, r)), key
        assert rows_equal(self.d_text.view(R, Lb), _to(np.frombuffer(self.block, dtype=np.uint8))), "the parse wrote into the text"


@pytest.mark.parametrize("where", ("sequence", "header", "record start"))
def test_fasta_parse_beyond_4gib(ctx, where):
    """Above the line: text positions (n_text > 2^32 + 64 MiB), the head and raw span offsets, `consumed`; the payload offsets
    pass 2^32 too where the block's payload is dense enough (asserted for what it is)."""
    p = Parsed(ctx, where)
    p.check()
    assert int(p.d_spans[0, -1, 0]) > LINE and int(p.d_spans[1, -1, 0]) > LINE
    del p


def test_fasta_write_beyond_4gib(ctx):
    """Above the line: the head spans, the text positions, the output offsets and the total (B2, first half); d_raw[h].off and
    d_head[h].off of the 64 records round byte 2^32 of the text, through d_src (second half)."""
    import torch
    from tests import fasta_sets as F
    block = H.block_for("sequence")
    one = F.host(block)
    head = [block[int(o):int(o + n)] for o, n in one["head"]]
    raw = [block[int(o):int(o + n)] for o, n in one["raw"]]
    body = [one["data"][int(a):int(b)].tobytes() for a, b in zip(one["offsets"][:-1], one["offsets"][1:])]
    written = [b">" + h + b"\n" + s + b"\n" for h, s in zip(head, body)]
    W = sum(len(w) for w in written)
    # (the written text is shorter than the text it was parsed from: no \r, no blank line; so the text is repeated until the
    # written one passes 2^32 + 64 MiB too.  The exact payload as byte capacity leaves room for the written text.)
    p = Parsed(ctx, "sequence", byte_capacity=lambda q: q.R * q.P, repeats=-(-(LINE + 64 * MIB) // W))
    assert p.status == (p.n_rec, p.R * p.P, p.n_text) and p.block == block
    R, r, P, Lb = p.R, p.r, p.P, p.Lb
    total = R * W
    assert total > LINE + 64 * MIB
    d_text_out = torch.empty(total, dtype=torch.uint8, device=_dev())
    d_out_off = torch.full((p.n_rec + 1,), -1, dtype=torch.int64, device=_dev())
    ctx.fasta_write_device(p.d_text, p.n_text, p.d_spans[0], p.n_rec, p.n_rec, d_text_out, total, d_out_off, d_body=p.d_out, d_body_offsets=p.d_off)
    assert ctx.fasta_write_status() == (total, 0)
    i = torch.arange(R, dtype=torch.int64, device=_dev())[:, None]
    w_off = np.concatenate([[0], np.cumsum([len(w) for w in written])]).astype(np.int64)
    assert torch.equal(d_out_off[:R * r].view(R, r), i * W + _to(w_off[:r])[None, :]) and int(d_out_off[R * r]) == total
    assert rows_equal(d_text_out.view(R, W), _to(np.frombuffer(b"".join(written), dtype=np.uint8))), "the text is not the block's records tiled"
    del d_text_out, d_out_off
    torch.cuda.empty_cache()
    # the 64 records round byte 2^32 of the text, their bodies from the raw spans
    mid = (LINE // Lb) * r
    src = np.arange(mid - 32, mid + 32, dtype=np.uint64)
    want = [b">" + head[int(k) % r] + b"\n" + raw[int(k) % r] + b"\n" for k in src]
    spans = p.d_spans[:, mid - 32:mid + 32, 0].cpu().numpy()
    assert (spans[:, 0] < LINE).all() and (spans[:, -1] > LINE).all()                    # head and raw offsets on both sides of the line
    small = sum(len(w) for w in want)
    d_small = torch.full((small + 64,), 0x3F, dtype=torch.uint8, device=_dev())
    d_small_off = torch.full((64 + 1 + 8,), -1, dtype=torch.int64, device=_dev())
    ctx.fasta_write_device(p.d_text, p.n_text, p.d_spans[0], p.n_rec, 64, d_small, small, d_small_off, d_raw=p.d_spans[1], d_src=_to(_i64(src)), n_src=64)
    assert ctx.fasta_write_status() == (small, 0)
    got = d_small.cpu().numpy()
    assert got[:small].tobytes() == b"".join(want) and (got[small:] == 0x3F).all()
    off = d_small_off.cpu().numpy()
    assert off[:65].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and (off[65:] == -1).all()
    del p, d_small, d_small_off


# ---- B3 / B4: the compacts and the gather with more than 4 GiB of output ---------------------------------------------------------
N, L = 4_400_000, 999


def big_batch(ctx):
    import torch
    d_bytes = torch.empty(N * L, dtype=torch.uint8, device=_dev())
    d_offs = torch.empty(N + 1, dtype=torch.int64, device=_dev())
    ctx.synth_fill_device(77, 0, N * L, d_bytes)
    ctx.fixed_offsets_device(0, L, N, d_offs)
    return d_bytes, d_offs


def test_uniq_compact_keeps_more_than_4gib(ctx):
    """Above the line: the input offsets behind record 4.3 M, the output offsets and positions, kept_bytes."""
    import torch
    assert N * L > LINE
    d_bytes, d_offs = big_batch(ctx)
    i = torch.arange(N, dtype=torch.int64, device=_dev())
    d_fs = torch.where(i % 97 == 0, i - 1, i)                                   # (-1 for i = 0: ~0 as uint64)
    kept = torch.nonzero(i % 97 != 0).view(-1)
    dropped = torch.nonzero(i % 97 == 0).view(-1)
    m = int(kept.numel())
    d_out = torch.empty(N * L, dtype=torch.uint8, device=_dev())
    d_out_off = torch.full((N + 1,), -1, dtype=torch.int64, device=_dev())
    d_src, d_dup_src, d_dup_first = (torch.full((N,), -7, dtype=torch.int64, device=_dev()) for _ in range(3))
    ctx.uniq_compact_device(d_bytes, d_offs, N, d_fs, d_out, d_out_off, d_src, d_dup_src=d_dup_src, d_dup_first=d_dup_first)
    n_kept, kept_bytes = ctx.uniq_compact_status()
    assert (n_kept, kept_bytes) == (m, m * L) and kept_bytes > LINE
    assert torch.equal(d_out_off[:m + 1], torch.arange(m + 1, dtype=torch.int64, device=_dev()) * L) and bool((d_out_off[m + 1:] == -1).all())
    assert torch.equal(d_src[:m], kept) and bool((d_src[m:] == -7).all())
    assert torch.equal(d_dup_src[:N - m], dropped) and torch.equal(d_dup_first[:N - m], dropped - 1) and bool((d_dup_src[N - m:] == -7).all())
    rows_in, rows_out = d_bytes.view(N, L), d_out[:m * L].view(m, L)
    for a in range(0, m, 1 << 19):
        assert torch.equal(rows_out[a:a + (1 << 19)], rows_in.index_select(0, kept[a:a + (1 << 19)])), a
    del d_bytes, d_out, rows_in, rows_out


def test_monomers_compact_keeps_more_than_4gib(ctx):
    """Above the line: the input offsets, the output offsets (a cumulative sum of 4.4 M ends) and positions, kept_bytes."""
    import torch
    d_bytes, d_offs = big_batch(ctx)
    i = torch.arange(N, dtype=torch.int64, device=_dev())
    ends = L - i % 3
    d_end = ends.to(torch.int32)
    d_out = torch.empty(N * L, dtype=torch.uint8, device=_dev())
    d_out_off = torch.full((N + 1,), -1, dtype=torch.int64, device=_dev())
    d_src = torch.full((N,), -7, dtype=torch.int64, device=_dev())
    d_kept = torch.full((N,), -7, dtype=torch.int32, device=_dev())
    ctx.monomers_compact_device(d_bytes, d_offs, N, d_end, d_out, d_out_off, d_src, d_kept_end=d_kept)
    n_kept, kept_bytes = ctx.monomers_status()
    total = int(ends.sum())
    assert (n_kept, kept_bytes) == (N, total) and kept_bytes > LINE
    exp_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=_dev()), torch.cumsum(ends, 0)])
    assert torch.equal(d_out_off, exp_off) and torch.equal(d_src, i) and torch.equal(d_kept, d_end)
    # record by record, the 4096 records round byte 2^32 of the output
    mid = int(torch.searchsorted(exp_off, torch.tensor([LINE], dtype=torch.int64, device=_dev()))[0])
    lo = mid - 2048
    assert int(exp_off[lo]) < LINE < int(exp_off[lo + 4096])
    for k in range(3):                                                          # the records of one residue class have one length
        idx = torch.arange(lo + (k - lo) % 3, lo + 4096, 3, dtype=torch.int64, device=_dev())
        n = L - k
        cols = torch.arange(n, dtype=torch.int64, device=_dev())[None, :]
        assert torch.equal(d_out[(exp_off[idx][:, None] + cols)], d_bytes[(idx * L)[:, None] + cols]), k
    # as a whole: three records take 3L - 3 output bytes; one strided view per residue class
    G = N // 3
    out3, in3 = d_out[:G * (3 * L - 3)].view(G, 3 * L - 3), d_bytes[:G * 3 * L].view(G, 3 * L)
    at = 0
    for k in range(3):
        n = L - k
        for a in range(0, G, 1 << 19):
            assert torch.equal(out3[a:a + (1 << 19), at:at + n], in3[a:a + (1 << 19), k * L:k * L + n]), (k, a)
        at += n
    for rec in range(3 * G, N):                                                 # (N is no multiple of 3: the last records)
        a = int(exp_off[rec])
        assert torch.equal(d_out[a:a + L - rec % 3], d_bytes[rec * L:rec * L + L - rec % 3])
    del d_bytes, d_out, out3, in3


def complement(t):
    """A <-> T, C <-> G of a pure ACGT tensor, with four masks."""
    import torch
    A, C, G, T = b"ACGT"
    return torch.where(t == A, T, torch.where(t == C, G, torch.where(t == G, C, torch.where(t == T, A, t))))


def test_revcomp_of_more_than_4gib(ctx):
    """Above the line: the input offsets, the window index times the record length, the output offsets and positions."""
    import torch
    d_bytes, d_offs = big_batch(ctx)
    d_win = torch.empty(24 * N, dtype=torch.uint8, device=_dev())
    d_out = torch.empty(N * L, dtype=torch.uint8, device=_dev())
    d_out_off = torch.full((N + 1,), -1, dtype=torch.int64, device=_dev())
    ctx.windows_of_records_device(d_offs, N, "revcomp", d_win)
    ctx.windows_gather_device(d_bytes, d_offs, N, d_win, N, d_out, N * L, d_out_off)
    assert ctx.windows_status() == (N * L, 0) and N * L > LINE
    assert torch.equal(d_out_off, torch.arange(N + 1, dtype=torch.int64, device=_dev()) * L)
    rows_in, rows_out = d_bytes.view(N, L), d_out.view(N, L)
    for a in range(0, N, 1 << 18):
        assert torch.equal(rows_out[a:a + (1 << 18)], complement(rows_in[a:a + (1 << 18)].flip(1))), a
    del d_bytes, d_out, rows_in, rows_out


def three_records():
    rng = np.random.default_rng(999)
    recs = [H.decoy(int(rng.integers(1 << 30)), n).tobytes() for n in (999, 1000, 16)]
    return recs, H.pack(recs)


def periodic(d_out, a, length, first):
    """d_out[a, a + length) repeats `first` (a numpy period), the last repeat cut short."""
    import torch
    p = len(first)
    d_first = _to(first)
    whole = length // p
    assert whole > 1 and rows_equal(d_out[a:a + whole * p].view(whole, p), d_first, chunk=1 << 20)
    return torch.equal(d_out[a + whole * p:a + length], d_first[:length - whole * p])


def test_windows_longer_than_4gib(ctx):
    """Above the line: a window's length, the position inside a window, the output offsets and the total; the start 2^32 - 1."""
    import torch
    from tests import windows_ref as R
    recs, (data, offs) = three_records()
    rows = [(LINE + 12345, 0, 998, 1), (2 ** 31 + 7, 1, 2 ** 32 - 1, 0), (100, 2, 5, 1)]
    wins = R.windows(rows)
    total = sum(r[0] for r in rows)
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=_dev())
    d_out[total:] = 0x3F
    d_out_off = torch.full((4 + 4,), -1, dtype=torch.int64, device=_dev())
    ctx.windows_gather_device(_to(data), _to(_i64(offs)), 3, _to(wins.view(np.uint8)), 3, d_out, total, d_out_off)
    assert ctx.windows_status() == (total, 0)
    exp_off = np.concatenate([[0], np.cumsum([r[0] for r in rows])])
    assert d_out_off.cpu().numpy().tolist() == exp_off.tolist() + [-1] * 4 and bool((d_out[total:] == 0x3F).all())
    for k, (length, rec, start, strand) in enumerate(rows):
        n = len(recs[rec])
        first = R.gather(data, offs, R.windows([(n, rec, start, strand)]))[0]
        assert len(first) == n
        if length > 2 * n:
            assert periodic(d_out, int(exp_off[k]), length, first), k
    short = R.gather(data, offs, wins[2:])[0]
    assert np.array_equal(d_out[int(exp_off[2]):total].cpu().numpy(), short)
    del d_out


def test_proteins_of_more_than_4gib(ctx):
    """Above the line: residue positions inside a window (3 t passes 2^32 before t does), out_offsets[2] and the total."""
    import torch
    from tests import test_translate_gpu as TG
    from tests import translate_ref as T
    from tests import translate_sets as TS
    from tests import windows_ref as R
    recs, (data, offs) = three_records()
    rows = [(3 * (2 ** 31 + 1000), 0, 998, 1), (3 * (2 ** 31 + 11), 1, 2 ** 32 - 1, 0), (50, 2, 5, 1)]
    wins = R.windows(rows)
    residues = [r[0] // 3 for r in rows]
    total = sum(residues)
    assert total > LINE
    aa, unknown, _ = TS.CODES[0]
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=_dev())
    d_out[total:] = 0x3F
    d_out_off = torch.full((4 + 4,), -1, dtype=torch.int64, device=_dev())
    ctx.windows_translate_device(_to(data), _to(_i64(offs)), 3, _to(wins.view(np.uint8)), 3, d_out, total, d_out_off, params=TG.params((aa, unknown, True)))
    assert ctx.translate_status() == (total, 0)
    exp_off = np.concatenate([[0], np.cumsum(residues)])
    assert d_out_off.cpu().numpy().tolist() == exp_off.tolist() + [-1] * 4 and bool((d_out[total:] == 0x3F).all())
    for k, (length, rec, start, strand) in enumerate(rows):
        n = len(recs[rec])
        p = n // 3 if n % 3 == 0 else n                                        # residues until the codons repeat
        plain = T.windows_translate(data, offs, R.windows([(3 * p, rec, start, strand)]), aa, unknown, False)[0]
        as_m = T.windows_translate(data, offs, R.windows([(3 * p, rec, start, strand)]), aa, unknown, True)[0]
        assert len(plain) == p and as_m[0] == ord("M") != plain[0] and np.array_equal(as_m[1:], plain[1:])
        a = int(exp_off[k])
        got0 = d_out[a:a + min(p, residues[k])].cpu().numpy()
        assert np.array_equal(got0, as_m[:len(got0)]), k                           # first_as_m: residue 0 of the window ...
        if residues[k] > 2 * p:
            assert periodic(d_out, a + p, residues[k] - p, plain), k                 # ... and of no later period
    del d_out
