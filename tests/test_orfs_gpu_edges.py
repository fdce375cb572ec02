"""GPU: the ORF kernels where the host build of the per-lane routine does not reach.  The scan across tiles and across
chunks of tile sums, the emit kernel's sort on both sides of its insertion / heapsort switch, canaries and the capacity,
a batch past 4 GiB, device views at every alignment with codons around them, exact filter boundaries, and back-to-back
batches on one context.  Every record and every field against the C restatement (tests/orfs_ref.c)."""
import random

import numpy as np
import pytest

from tests import orfs_ref as R
from tests.test_orfs_cpu import SCAN_COUNTS, _pack, filter_boundary_cases, kernel_constants, sort_switch_records

pytestmark = pytest.mark.gpu

FIELDS = ("start", "stop", "length", "wraps", "strand")
POISON = 0xA5                                    # ORF buffer canary byte
SENTINEL = 0x5A5A5A5A5A5A5A5A                    # offsets canary


@pytest.fixture(scope="module")
def ctx():
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    # torch's stream, not the ctx's own non-blocking one: the tests fill their canaried outputs with torch.full right before
    # the call, and a fill still running on another stream lands on top of what the count kernel wrote (seen once at
    # 8,388,608 records: offsets[0] and the total came back as canaries)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def _dev():
    import torch
    return torch.device("cuda", 0)


def _same(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0] if len(got) == len(exp) else []
        k = int(bad[0]) if len(bad) else -1
        raise AssertionError("%s differs (len %d vs %d), first at %d: %r vs %r" %
                             (what, len(got), len(exp), k, got[k] if k >= 0 else None, exp[k] if k >= 0 else None))


def _same_orfs(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for f in FIELDS:
        _same(got[f], exp[f], "%s: %s" % (what, f))


def check_host(ctx, seqs, **kw):
    """ctx.orfs_batch (the host form) against the restatement; returns the total."""
    d, o = _pack(seqs)
    eo, e = R.orfs_batch(d, o, threads=16, **kw)
    got = ctx.orfs_batch(d, o, **kw)
    _same(got["offsets"], eo, "offsets %r" % kw)
    for f in FIELDS:
        _same(got[f], e[f], "%s %r" % (f, kw))
    return len(e)


def _device_offsets(ctx, d_bytes, d_offsets, n, d_oo, **kw):
    """Count + scan only (no ORF buffer, capacity 0: nothing is emitted); returns the total circkit_orfs_status reports
    (with CIRCKIT_ERR_OOM when it is not 0)."""
    import ctypes
    ctx.orfs_batch_device(d_bytes, d_offsets, n, d_oo, None, 0, **kw)
    t = ctypes.c_uint64(0)
    rc = ctx._lib.circkit_orfs_status(ctx._h, ctypes.byref(t))
    assert rc == (0 if t.value == 0 else -5), (rc, t.value)
    return t.value


def check_device(ctx, d_bytes, d_offsets, n, eo, e, **kw):
    """The device form on n records into outputs with canaries past their ends: the offsets, every ORF, the total, and
    nothing written past offsets[n] or past the last ORF.  The offsets are checked from a count + scan run first, so that
    offsets a broken scan got wrong fail here and never reach the emit kernel."""
    import torch
    total = int(eo[n])
    d_oo = torch.full((n + 1 + 64,), SENTINEL, dtype=torch.int64, device=_dev())
    assert _device_offsets(ctx, d_bytes, d_offsets, n, d_oo, **kw) == total, "total of %d records" % n
    oo = d_oo.cpu().numpy()
    _same(oo[:n + 1].view(np.uint64), eo[:n + 1], "offsets of %d records (count + scan)" % n)
    assert (oo[n + 1:] == SENTINEL).all(), "written past offsets[n]"
    d_orfs = torch.full(((total + 64) * 24,), POISON, dtype=torch.uint8, device=_dev())
    ctx.orfs_batch_device(d_bytes, d_offsets, n, d_oo, d_orfs, total, **kw)
    assert ctx.orfs_status() == total
    oo = d_oo.cpu().numpy()
    _same(oo[:n + 1].view(np.uint64), eo[:n + 1], "offsets of %d records" % n)
    assert (oo[n + 1:] == SENTINEL).all(), "written past offsets[n]"
    raw = d_orfs.cpu().numpy()
    assert (raw[total * 24:] == POISON).all(), "written past the last ORF"
    _same_orfs(raw[:total * 24].view(R.ORF_DTYPE), e[:total], "%d records" % n)


# ---- 1. the scan: both sides of every edge ---------------------------------------------------------------------------
def scan_batch(n):
    """n records of 2-12 symbols laid out by scan tiles, in turn: a tile of zero-ORF records, a tile where every record
    has ORFs, a tile of random records, and a tile of zero-ORF records but for a dense record (4 ORFs) at its first and
    last slot.  The last three kinds have that dense record at both ends.  Tile 0 is one where every record has ORFs, so
    that the counts vary at the workgroup edges and the first tile edge.  Returns (bytes, offsets)."""
    tile_len = kernel_constants()["SCAN_TILE"]
    rng = np.random.default_rng(21)
    idx = np.arange(n, dtype=np.int64)
    kind = (idx // tile_len) % 4
    kind[:tile_len] = 1
    slot = idx % tile_len
    lens = rng.integers(2, 13, n)
    dense = (kind != 0) & ((slot == 0) | (slot == tile_len - 1))
    lens[kind == 1] = np.maximum(lens[kind == 1], 3)
    lens[dense] = 12
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    data = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(offs[-1]), dtype=np.uint8)]
    data[np.repeat((kind == 0) | ((kind == 3) & ~dense), lens)] = ord("C")
    starts = offs[:-1].astype(np.int64)
    for k, b in enumerate(b"ATG"):
        data[starts[kind == 1] + k] = b
    for k, b in enumerate(b"ATGATGATGATG"):
        data[starts[dense] + k] = b
    return data, offs


def test_scan_edges_every_record(ctx):
    """Batches of SCAN_COUNTS records: both sides of a workgroup, of a scan tile and of one chunk of 1024 tile sums
    (8,388,608 records), then a second chunk of one tile and a third chunk.  mode 1, min_length 0: every offset and every
    ORF."""
    import torch
    c = kernel_constants()
    N = SCAN_COUNTS[-1]
    assert N > 2 * c["SCAN_WG"] * c["SCAN_TILE"]                  # three chunks in scan_sums
    data, offs = scan_batch(N)
    kw = dict(mode=1, min_length=0, require_stop=False, strands=3)
    eo, e = R.orfs_batch(data, offs, threads=16, **kw)
    tile_sums = np.diff(eo[::c["SCAN_TILE"]].astype(np.int64))
    assert (tile_sums == 0).any() and (tile_sums > 0).any()
    assert all(eo[n] > 0 for n in SCAN_COUNTS)
    for edge in (c["ORF_WG"], c["SCAN_TILE"]):                   # every record around these edges has ORFs, in varying number
        counts = np.diff(eo[edge - 3:edge + 4].astype(np.int64))
        assert (counts > 0).all() and len(set(counts.tolist())) > 1, (edge, counts)
    d_bytes = torch.from_numpy(data).to(_dev())
    d_offs = torch.from_numpy(offs.view(np.int64)).to(_dev())
    for n in SCAN_COUNTS:
        check_device(ctx, d_bytes, d_offs, n, eo, e, **kw)


# ---- 2. the emit kernel's sort -----------------------------------------------------------------------------------------
def test_sort_switch_both_modes_and_strands(ctx):
    """Runs of exactly 31, 32, 33, 64 and 3000 ORFs per strand, equal lengths across frames (tests/test_orfs_cpu.py
    sort_switch_records): the insertion sort, the heapsort and its ties, on the GPU."""
    seqs = sort_switch_records()
    for mode in (0, 1):
        for strands in (1, 2, 3):
            assert check_host(ctx, seqs, mode=mode, strands=strands, min_length=0) > 0


# ---- 3. canaries and the capacity ----------------------------------------------------------------------------------------
def test_canaries_and_capacity(ctx):
    """Views into larger buffers, with guards before and after the input bytes, the offsets and both outputs.  Capacity =
    total, total - 1, 0 and no ORF buffer.  The records that fit are written exactly and nothing else is, the input is
    left as it was, and orfs_status reports -5 and the total."""
    import torch
    import circkit_amd
    rng = random.Random(61)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(2, 3000))) for _ in range(3000)]
    d, o = _pack(seqs)
    n = len(seqs)
    eo, e = R.orfs_batch(d, o, threads=16)
    total = int(eo[-1])
    assert eo[-2] < total                                             # the last record has ORFs: total - 1 cuts its run
    G = 4096
    dev = _dev()
    pad = np.frombuffer(b"ATGTAATAG" * (G // 9 + 1), dtype=np.uint8)[:G]
    bytes_buf = torch.from_numpy(np.concatenate([pad, d, pad])).to(dev)
    offs_buf = torch.full((G + n + 1 + G,), SENTINEL, dtype=torch.int64, device=dev)
    offs_buf[G:G + n + 1] = torch.from_numpy((o + G).view(np.int64)).to(dev)
    in_before = (bytes_buf.cpu().numpy().copy(), offs_buf.cpu().numpy().copy())
    oo_buf = torch.empty(G + n + 1 + G, dtype=torch.int64, device=dev)
    orf_buf = torch.empty((G + total + G) * 24, dtype=torch.uint8, device=dev)
    for cap in (total, total - 1, 0, None):
        oo_buf.fill_(SENTINEL)
        orf_buf.fill_(POISON)
        ctx.orfs_batch_device(bytes_buf, offs_buf[G:], n, oo_buf[G:G + n + 1], None if cap is None else orf_buf[G * 24:],
                              0 if cap is None else cap)
        if cap == total:
            assert ctx.orfs_status() == total
        else:
            with pytest.raises(circkit_amd.CirckitError) as ex:
                ctx.orfs_status()
            assert ex.value.code == -5 and str(total) in str(ex.value), (cap, str(ex.value))
        oo = oo_buf.cpu().numpy()
        assert (oo[:G] == SENTINEL).all() and (oo[G + n + 1:] == SENTINEL).all(), cap
        _same(oo[G:G + n + 1].view(np.uint64), eo, "offsets, capacity %s" % cap)
        raw = orf_buf.cpu().numpy()
        assert (raw[:G * 24] == POISON).all() and (raw[(G + total) * 24:] == POISON).all(), cap
        body = raw[G * 24:(G + total) * 24]
        fit = int(eo[np.searchsorted(eo, cap, side="right") - 1]) if cap else 0     # the ORFs of the records that fit
        _same_orfs(body[:fit * 24].view(R.ORF_DTYPE), e[:fit], "capacity %s" % cap)
        assert (body[fit * 24:] == POISON).all(), ("written past the records that fit", cap, fit)
        b_after, o_after = bytes_buf.cpu().numpy(), offs_buf.cpu().numpy()
        assert np.array_equal(b_after, in_before[0]) and np.array_equal(o_after, in_before[1]), "input changed"


# ---- 4. a batch past 4 GiB ---------------------------------------------------------------------------------------------
def test_batch_past_4gib_every_record(ctx):
    """4.4M records of 1 kb (4.4 GB), generated on the device and, for the restatement, on the host: every record.  The
    last record starts at byte 4,399,999,000, past 2^32."""
    import torch
    from oracle import oracle as O
    n, L = 4_400_000, 1000
    assert (n - 1) * L == 4_399_999_000 > 2 ** 32
    d_bytes = torch.empty(n * L, dtype=torch.uint8, device=_dev())
    ctx.synth_fill_device(9, 0, n * L, d_bytes)
    d_offs = torch.arange(n + 1, dtype=torch.int64, device=_dev()) * L
    h = O.synth_fill(9, 0, n * L)
    kw = dict(min_length=75, require_stop=True)
    eo, e = R.orfs_batch(h, np.arange(n + 1, dtype=np.uint64) * L, threads=16, **kw)
    del h
    assert int(eo[-1]) > n and eo[-1] > eo[-2]                         # the last record has ORFs
    check_device(ctx, d_bytes, d_offs, n, eo, e, **kw)


# ---- 5. offset and alignment views ----------------------------------------------------------------------------------------
def test_offset_views_every_shift(ctx):
    """The device form with offsets[0] at every shift 0-15 from a 256-byte boundary.  Records around multiples of 16 and
    64, of 1-2 kb and of 100 kb; start and stop codons in the bytes before the first record and after the last."""
    import torch
    rng = random.Random(71)
    lens = [2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193]
    lens += [rng.randint(1000, 2000) for _ in range(6)] + [100_003, 5]
    units = [b"ATG", b"TAA", b"TGA", b"TAG", b"CAT", b"A", b"C", b"G", b"T"]
    seqs = [b"".join(rng.choice(units) for _ in range(L))[:L] for L in lens]
    d, o = _pack(seqs)
    n = len(seqs)
    pad = np.frombuffer(b"ATGATGTAATAGTGACAT" * 32, dtype=np.uint8)
    configs = [dict(), dict(mode=1, min_length=0, max_wraps=3), dict(mode=0, min_length=0, strands=2)]
    expect = [R.orfs_batch(d, o, threads=16, **kw) for kw in configs]
    for shift in range(16):
        head = pad[:256 + shift]
        buf = torch.from_numpy(np.concatenate([head, d, pad])).to(_dev())
        d_offs = torch.from_numpy((o + len(head)).view(np.int64)).to(_dev())
        for kw, (eo, e) in zip(configs, expect):
            check_device(ctx, buf, d_offs, n, eo, e, **kw)


# ---- 6. exact filter boundaries ------------------------------------------------------------------------------------------
def test_exact_filter_boundaries(ctx):
    """min_ratio at length / L and its neighbours on records of prime lengths, min_length at length - 3 and around it and
    near 2^64, min_wraps above max_wraps, max_wraps of 4 and 2^32 - 1 (tests/test_orfs_cpu.py filter_boundary_cases)."""
    seqs, cases, _ = filter_boundary_cases()
    for kw in cases:
        check_host(ctx, seqs, **kw)


# ---- 7. back-to-back batches on one context -----------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["ctx", "torch_side"])
def test_back_to_back_batches(stream):
    """A fresh context, whose tile-sum buffer has not grown yet, with no sync in between: a small batch, a canonicalize
    batch, then a batch large enough to grow the tile sums, with other params and into other buffers.  One orfs_status
    reports the second.  On the context's own stream and on a torch side stream."""
    import torch
    import circkit_amd
    from oracle import oracle as O
    dev = _dev()
    c = circkit_amd.Context(0)
    try:
        if stream == "torch_side":
            side = torch.cuda.Stream(device=dev)
            c.set_stream(side.cuda_stream)
        rng = random.Random(81)
        small = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(2, 400))) for _ in range(100)]
        big = [bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(2, 40))) for _ in range(3 * kernel_constants()["SCAN_TILE"] + 7)]
        batches = []
        for seqs, kw in ((small, dict(mode=0)), (big, dict(mode=1, min_length=0, start_codons=["ATG", "CTG"], strands=2))):
            d, o = _pack(seqs)
            eo, e = R.orfs_batch(d, o, threads=16, **kw)
            t = int(eo[-1])
            batches.append(dict(n=len(seqs), kw=kw, eo=eo, e=e, total=t, d=torch.from_numpy(d.copy()).to(dev),
                                o=torch.from_numpy(o.view(np.int64)).to(dev),
                                oo=torch.full((len(seqs) + 1,), SENTINEL, dtype=torch.int64, device=dev),
                                orfs=torch.full(((t + 1) * 24,), POISON, dtype=torch.uint8, device=dev)))
        a, b = batches
        assert a["total"] != b["total"]
        cd, co = _pack(small)
        c_bytes, c_offs = torch.from_numpy(cd.copy()).to(dev), torch.from_numpy(co.view(np.int64)).to(dev)
        c_out = torch.zeros(len(cd), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        c.orfs_batch_device(a["d"], a["o"], a["n"], a["oo"], a["orfs"], a["total"], **a["kw"])
        c.canonicalize_batch_device(c_bytes, c_offs, len(small), out_bytes=c_out)
        c.orfs_batch_device(b["d"], b["o"], b["n"], b["oo"], b["orfs"], b["total"], **b["kw"])
        assert c.orfs_status() == b["total"]
        for x in (a, b):
            _same(x["oo"].cpu().numpy().view(np.uint64), x["eo"], "offsets %r" % x["kw"])
            raw = x["orfs"].cpu().numpy()
            assert (raw[x["total"] * 24:] == POISON).all()
            _same_orfs(raw[:x["total"] * 24].view(R.ORF_DTYPE), x["e"], "%r" % x["kw"])
        exp_c, _ = O.canonicalize_batch(cd, co, True, False, threads=16)
        assert np.array_equal(c_out.cpu().numpy(), exp_c)
    finally:
        c.close()
