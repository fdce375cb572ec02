"""Every output combination of the batch entry points, on every kernel path (run with -m gpu).

include/circkit.h makes each output of circkit_canonicalize_batch_device nullable, in any combination, and defines
circkit_lmsr_batch_device as the lib crate's lmsr() for a whole batch (forward strand, either output nullable).  The outputs
asked for decide which builds launch_canon runs (index / strand / forward-only: the index builds, never the mixed-length
kernel; a hash without bytes: per-record views; 1009..2032-symbol batches that want a hash and nothing per record: mode 3),
so every cell of {15 output subsets + lmsr x 3} x {one record set per route, tests/seqsets.py KINDS} is run here, each kind
three times in a row (the first batch of a kind meets the previous kind's mode guess, the third a settled one), against the
oracle record for record, with canaries around every buffer."""
import numpy as np
import pytest

from tests import seqsets

pytestmark = pytest.mark.gpu

OUTPUTS = ("b", "i", "s", "h")                      # bytes, index, strand, xxh3
SUBSETS = ["".join(o for k, o in enumerate(OUTPUTS) if m >> k & 1) for m in range(1, 16)]
LMSR_SUBSETS = ["b", "i", "bi"]
# kinds in an order that changes the mode at (almost) every step, so that the first batch of each kind runs on a wrong guess
KIND_ORDER = ["k1kb", "kmixed", "kshort", "ktwo", "kalpha", "klong", "kodd"]
PAD, SPARE = 64, 64                                 # canary bytes around the payload; spare entries behind each per-record output
S_BYTE, S_IDX, S_STRAND, S_HASH = 0xA5, 0x5A5A5A5A, 0xEE, 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.lib()
    return oracle


@pytest.fixture(scope="module")
def gpu():
    import torch
    import circkit_amd
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield ctx, torch.device("cuda", 0)
    ctx.close()


class Batch:
    """One record set on the device in two layouts: plain, and with offsets[0] = 24 and the payload and output pointers at an
    odd address (shift 5).  Canary bytes around the payload in both, sentinel-filled outputs with SPARE entries behind."""

    def __init__(self, seqs, dev, O, lmsr_oracle=True):
        import torch
        self.seqs = seqs
        self.data, self.offs = seqsets.pack(seqs)
        self.n, self.nb = len(seqs), len(self.data)
        self.exp = O.canonicalize_batch_aux(self.data, self.offs, True, True, True, True, threads=16)   # bytes, xxh3, index, strand
        self.lexp = O.lmsr_batch(self.data, self.offs, threads=16) if lmsr_oracle else None
        self.layouts = []
        for shift, lead in ((0, 0), (5, 24)):
            raw = np.full(PAD + shift + lead + self.nb + PAD, 0xC3, dtype=np.uint8)
            raw[PAD + shift + lead:PAD + shift + lead + self.nb] = self.data
            d_raw = torch.from_numpy(raw).to(dev)
            d_off = torch.from_numpy((self.offs + np.uint64(lead)).astype(np.int64)).to(dev)
            self.layouts.append(dict(shift=shift, lead=lead, d_raw=d_raw, d_raw0=d_raw.clone(), d_off=d_off, d_off0=d_off.clone(),
                                     d_out_raw=torch.empty_like(d_raw)))
        self.d_idx = torch.empty(self.n + SPARE, dtype=torch.int32, device=dev)
        self.d_strand = torch.empty(self.n + SPARE, dtype=torch.uint8, device=dev)
        self.d_hash = torch.empty(self.n + SPARE, dtype=torch.int64, device=dev)

    def run(self, ctx, outs, layout, lmsr=False):
        """One call with the outputs named in `outs` (b, i, s, h); returns what came back (numpy), canaries checked."""
        import torch
        L = self.layouts[layout]
        base = PAD + L["shift"]
        L["d_out_raw"].fill_(S_BYTE)
        self.d_idx.fill_(S_IDX)
        self.d_strand.fill_(S_STRAND)
        self.d_hash.fill_(S_HASH)
        d_bytes, d_out = L["d_raw"][base:], L["d_out_raw"][base:]
        ob = d_out if "b" in outs else None
        oi = self.d_idx if "i" in outs else None
        if lmsr:
            ctx.lmsr_batch_device(d_bytes, L["d_off"], self.n, out_bytes=ob, out_index=oi)
        else:
            ctx.canonicalize_batch_device(d_bytes, L["d_off"], self.n, out_bytes=ob, out_index=oi,
                                          out_strand=self.d_strand if "s" in outs else None, out_xxh3=self.d_hash if "h" in outs else None)
        mode = ctx.last_batch_mode()                                   # (synchronizes)
        status = ctx.batch_status()
        torch.cuda.synchronize()
        assert torch.equal(L["d_raw"], L["d_raw0"]) and torch.equal(L["d_off"], L["d_off0"]), "the input was written"
        out_raw = L["d_out_raw"].cpu().numpy()
        lo, hi = base + L["lead"], base + L["lead"] + self.nb
        assert (out_raw[:lo] == S_BYTE).all() and (out_raw[hi:] == S_BYTE).all(), "bytes written outside [offsets[0], offsets[n])"
        idx, strand, hs = self.d_idx.cpu().numpy().view(np.uint32), self.d_strand.cpu().numpy(), self.d_hash.cpu().numpy().view(np.uint64)
        for name, arr, s in (("index", idx, S_IDX), ("strand", strand, S_STRAND), ("xxh3", hs, S_HASH)):
            assert (arr[self.n:] == s).all(), "%s written past record n - 1" % name
        return dict(mode=mode, status=status, b=out_raw[lo:hi], i=idx[:self.n], s=strand[:self.n], h=hs[:self.n])

    def check(self, got, outs, lmsr=False, what=""):
        exp_b, exp_h, exp_i, exp_s = self.exp
        if lmsr:
            exp_b, exp_i = self.lexp
        if "b" in outs:
            if not np.array_equal(got["b"], exp_b):
                bad = [k for k in range(self.n) if not np.array_equal(got["b"][self.offs[k]:self.offs[k + 1]], exp_b[self.offs[k]:self.offs[k + 1]])]
                raise AssertionError("%s bytes: %d records differ, first %s (lengths %s)" % (what, len(bad), bad[:5], [len(self.seqs[k]) for k in bad[:5]]))
        else:
            assert (got["b"] == S_BYTE).all(), "%s: bytes written although none were asked for" % what
        for key, name, exp in (("i", "index", exp_i), ("s", "strand", exp_s), ("h", "xxh3", exp_h)):
            if key in outs:
                bad = np.nonzero(got[key] != exp)[0]
                assert len(bad) == 0, "%s %s: %d records differ, first %s (lengths %s)" % (what, name, len(bad), bad[:5].tolist(),
                                                                                         [len(self.seqs[k]) for k in bad[:5]])
            else:
                sentinel = {"i": S_IDX, "s": S_STRAND, "h": S_HASH}[key]
                assert (got[key] == sentinel).all(), "%s: %s written although it was not asked for" % (what, name)


@pytest.fixture(scope="module")
def kinds(gpu, O):
    _, dev = gpu
    return {k: Batch(seqsets.KINDS[k](), dev, O) for k in KIND_ORDER}


def _expect_mode(kind, got, outs, lmsr, what):
    want = seqsets.kind_mode(kind, "h" in outs, "i" in outs, "s" in outs, lmsr)
    if want is None:
        assert got in (1, 2, 3), what
    else:
        assert got == want, "%s: mode %d, expected %d" % (what, got, want)


@pytest.mark.parametrize("outs", SUBSETS)
def test_device_batch_every_output_subset_every_kind(gpu, kinds, outs):
    """circkit_canonicalize_batch_device with exactly the outputs in `outs`, every kind three times in a row (a wrong mode guess,
    then a settled one; the middle call with offsets[0] != 0 and odd payload / output addresses)."""
    ctx, _ = gpu
    for kind in KIND_ORDER:
        B = kinds[kind]
        for rep in range(3):
            what = "%s/%s/rep%d" % (kind, outs, rep)
            got = B.run(ctx, outs, layout=rep == 1)
            assert got["status"] == 0, what
            _expect_mode(kind, got["mode"], outs, False, what)
            B.check(got, outs, what=what)


@pytest.mark.parametrize("outs", LMSR_SUBSETS)
def test_lmsr_batch_every_output_subset_every_kind(gpu, kinds, outs):
    """circkit_lmsr_batch_device (forward strand only: lmsr(record), lmsr_index(record)) against the forward-only oracle."""
    ctx, _ = gpu
    for kind in KIND_ORDER:
        B = kinds[kind]
        for rep in range(3):
            what = "lmsr %s/%s/rep%d" % (kind, outs, rep)
            got = B.run(ctx, outs, layout=rep == 1, lmsr=True)
            assert got["status"] == 0, what
            _expect_mode(kind, got["mode"], outs, True, what)
            B.check(got, outs, lmsr=True, what=what)


def _host_check(B, got, outs, what):
    exp_b, exp_h, exp_i, exp_s = B.exp
    for key, name, exp in (("b", "bytes", exp_b), ("i", "index", exp_i), ("s", "strand", exp_s), ("h", "xxh3", exp_h)):
        if key in outs:
            assert got[name] is not None and np.array_equal(got[name], exp), (what, name)
        else:
            assert got[name] is None


@pytest.mark.parametrize("kind", ["kshort", "ktwo", "kmixed"])
def test_host_batch_every_output_subset(gpu, kinds, kind):
    """circkit_canonicalize_batch: here the host sees the offsets and decides the mode itself (host_mode) -- every subset."""
    ctx, _ = gpu
    B = kinds[kind]
    for outs in SUBSETS:
        got = ctx.canonicalize_batch(B.data, B.offs, want_bytes="b" in outs, want_index="i" in outs, want_strand="s" in outs,
                                     want_xxh3="h" in outs)
        _host_check(B, {"bytes": got["bytes"], "index": got["index"], "strand": got["strand"], "xxh3": got["xxh3"]}, outs, "%s/%s" % (kind, outs))
        assert ctx.batch_status() == 0


def test_host_batch_in_parts_with_one_per_record_output(gpu, O):
    """A host batch of >= 32 MB goes through the device in parts (launch_canon with keep_status on every part behind the first)
    -- with the index alone and with the hash alone."""
    ctx, _ = gpu
    rng = np.random.default_rng(4242)
    lens = rng.integers(300, 2000, size=36000)
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    data = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=int(offs[-1]))]
    data[rng.integers(0, len(data), size=len(data) // 500)] = ord("N")
    assert offs[-1] >= 32 << 20
    _, exp_h, exp_i, _ = O.canonicalize_batch_aux(data, offs, False, True, True, False, threads=16)
    got = ctx.canonicalize_batch(data, offs, want_bytes=False, want_index=True)
    assert got["bytes"] is None and np.array_equal(got["index"], exp_i)
    assert ctx.batch_status() == 0
    got = ctx.canonicalize_batch(data, offs, want_bytes=False, want_xxh3=True)
    assert np.array_equal(got["xxh3"], exp_h)
    assert ctx.batch_status() == 0


def test_call_without_outputs_writes_nothing(gpu, kinds):
    """No output at all: OK, nothing written (the input included), status 0 -- on every kind; and the batch behind it, of
    another kind, with every output, is right."""
    ctx, _ = gpu
    for k, kind in enumerate(KIND_ORDER):
        B = kinds[kind]
        for layout in (0, 1):
            got = B.run(ctx, "", layout=layout)
            assert got["status"] == 0, kind
            B.check(got, "", what="no outputs " + kind)
            nxt = kinds[KIND_ORDER[(k + 1) % len(KIND_ORDER)]]
            got = nxt.run(ctx, "bish", layout=layout)
            assert got["status"] == 0
            nxt.check(got, "bish", what="behind a call without outputs")


def test_batch_of_only_empty_records(gpu, O):
    """n records, all of length 0 (offsets all equal; the payload pointer valid, no byte of it ever needed): every subset, and
    lmsr; index 0, strand 1 (the reference returns lmsr(revcomp) when the two are equal), XXH3 of the empty string."""
    ctx, dev = gpu
    B = Batch([b""] * 300, dev, O)
    for outs in SUBSETS:
        for layout in (0, 1):
            got = B.run(ctx, outs, layout=layout)
            assert got["status"] == 0
            B.check(got, outs, what="empty/" + outs)
    for outs in LMSR_SUBSETS:
        got = B.run(ctx, outs, layout=1, lmsr=True)
        B.check(got, outs, lmsr=True, what="empty lmsr/" + outs)
    assert (B.exp[2] == 0).all() and (B.exp[3] == 1).all()


def test_single_record_every_subset(gpu, O):
    """n = 1 on the device (the batch pipeline) and through the host entry point (launch_single for a record that fits the first
    tier), every subset, records of several routes."""
    ctx, dev = gpu
    rng = np.random.default_rng(77)
    recs = [seqsets._np_seq(rng, 1000), seqsets._np_seq(rng, 150), seqsets._np_seq(rng, 1500),
            seqsets._sprinkle(rng, seqsets._np_seq(rng, 900), 0.02), seqsets._np_seq(rng, 30000), b"ACGT" * 300, b""]
    for r in recs:
        B = Batch([r], dev, O)
        for outs in SUBSETS:
            got = B.run(ctx, outs, layout=1)
            assert got["status"] == 0
            B.check(got, outs, what="n=1 len %d/%s" % (len(r), outs))
            h = ctx.canonicalize_batch(B.data, B.offs, want_bytes="b" in outs, want_index="i" in outs, want_strand="s" in outs,
                                       want_xxh3="h" in outs)
            _host_check(B, h, outs, "host n=1 len %d/%s" % (len(r), outs))
        for outs in LMSR_SUBSETS:
            got = B.run(ctx, outs, layout=0, lmsr=True)
            B.check(got, outs, lmsr=True, what="n=1 lmsr len %d/%s" % (len(r), outs))


def test_xxh3_batch_device_on_raw_records(gpu, O):
    """circkit_xxh3_batch_device on arbitrary bytes (0..255), every length 0..2100 and around the multiples of 1024 up to 4 KiB
    -- XXH3's short classes, the 240 edge, the stripe and block boundaries -- at 16 payload alignments."""
    import torch
    ctx, dev = gpu
    rng = np.random.default_rng(99)
    lens = list(range(0, 2101)) + [m * k for k in (3, 4) for m in (1023, 1024, 1025)] + [1024 * k + d for k in (3, 4) for d in (-1, 1)]
    seqs = [bytes(rng.integers(0, 256, size=n).astype(np.uint8)) for n in lens]
    data, offs = seqsets.pack(seqs)
    exp = np.array([O.xxh3_64(s) for s in seqs], dtype=np.uint64)
    n = len(seqs)
    d_hash = torch.empty(n + SPARE, dtype=torch.int64, device=dev)
    for shift in range(16):
        raw = np.full(PAD + shift + len(data) + PAD, 0xC3, dtype=np.uint8)
        raw[PAD + shift:PAD + shift + len(data)] = data
        d_raw = torch.from_numpy(raw).to(dev)
        d_off = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_hash.fill_(S_HASH)
        ctx.xxh3_batch_device(d_raw[PAD + shift:], d_off, n, d_hash)
        torch.cuda.synchronize()
        got = d_hash.cpu().numpy().view(np.uint64)
        bad = np.nonzero(got[:n] != exp)[0]
        assert len(bad) == 0, (shift, [lens[k] for k in bad[:8]])
        assert (got[n:] == S_HASH).all(), shift
        assert np.array_equal(d_raw.cpu().numpy(), raw), shift
