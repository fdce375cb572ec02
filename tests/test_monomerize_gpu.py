"""GPU: circkit_monomerize_batch / _device and circkit_monomer_end_index against the C restatement (tests/mono_ref.c).
Every record of every batch is compared."""
import ctypes
import random

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    import circkit_amd
    c = circkit_amd.Context(0)
    yield c
    c.close()


def _dev():
    import torch
    return torch.device("cuda", 0)


def compare(exp, got, kw, seqs=None):
    assert got.dtype == np.uint32 and len(got) == len(exp)
    bad = np.nonzero(exp != got)[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%d of %d records differ under %r; first: record %d%s, expected %d, got %d" % (
            len(bad), len(exp), kw, i, "" if seqs is None else " (%d bytes: %r...)" % (len(seqs[i]), seqs[i][:60]), int(exp[i]), int(got[i])))


def check(ctx, data, offs, seqs=None, threads=16, **kw):
    exp = R.batch(data, offs, threads=threads, **kw)
    compare(exp, ctx.monomerize_batch(data, offs, **kw), kw, seqs)
    return exp


def check_seqs(ctx, seqs, **kw):
    data, offs = S.pack(seqs)
    return check(ctx, data, offs, seqs, **kw)


def device_batch(ctx, data, offs, shift=0, guard=64, **kw):
    """monomerize_batch_device on a view that starts `shift` bytes into its buffer, with sentinels round the output."""
    import torch
    n = len(offs) - 1
    buf = torch.from_numpy(np.concatenate([np.full(shift, 0x41, np.uint8), data, np.full(64, 0x41, np.uint8)])).to(_dev())
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(_dev())
    d_end = torch.full((guard + n + guard,), SENTINEL, dtype=torch.int32, device=_dev())
    ctx.monomerize_batch_device(buf[shift:], d_offs, n, d_end[guard:], **kw)
    ctx.synchronize()
    out = d_end.cpu().numpy().view(np.uint32)
    assert (out[:guard] == SENTINEL).all() and (out[guard + n:] == SENTINEL).all(), "wrote outside the output array"
    assert np.array_equal(buf[shift:shift + len(data)].cpu().numpy(), data), "wrote into its input"
    return out[guard:guard + n].copy()


@pytest.mark.parametrize("k", (1, 5, 10, 63))
def test_every_length_and_the_adversarial_set(ctx, k):
    """The sets of the emulator test, whole, under every cut-off, plain and sensitive."""
    seqs = S.every_length(random.Random(100 + k))
    seqs += [b"A" * n for n in (k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1)]
    seqs += S.adversarial(long_poly=20000)
    some = 0
    for kw in S.settings((k,)):
        some += int((check_seqs(ctx, seqs, **kw) != R.NONE).sum())
    assert some > 1000


def test_identity_boundaries(ctx):
    cases = S.identity_boundaries()
    for ident in S.IDENTITIES:
        sub = [c for c in cases if c[1] == ident]
        exp = check_seqs(ctx, [c[0] for c in sub], seed_len=5, min_identity=ident)
        assert [int(e) for e in exp] == [c[2] if c[4] else R.NONE for c in sub]
        check_seqs(ctx, [c[0] for c in sub], seed_len=5, min_identity=ident, sensitive=True)


ROLLING_SETTINGS = (dict(min_identity=0.95), dict(max_mismatch=0), dict(max_mismatch=5), dict(max_mismatch=0, sensitive=True),
                    dict(max_mismatch=5, sensitive=True))


def test_rolling_batch(ctx):
    """Monomers of 150..700 symbols repeated to 1000, 1 % substitutions: between 5 % and 95 % of the records monomerize under
    every setting used here (asserted from the restatement alone), so neither outcome goes untested.  The restatement's
    figures: identity 0.95 86.8 %, max-mismatch 0 10.6 % (plain and sensitive), 5 52.3 % (sensitive 59.9 %)."""
    data, offs = S.rolling(1, [1000] * 1500)
    for kw in ROLLING_SETTINGS:
        exp = check(ctx, data, offs, seed_len=10, **kw)
        frac = float((exp != R.NONE).mean())
        assert 0.05 < frac < 0.95, (kw, frac)


def test_rolling_batch_sensitive_identity(ctx):
    """The same batch under identity 0.95 with the sensitive form.  97.8 % of it monomerize then (the restatement's figure), so
    what is asserted here is that the sensitive pass changes between 5 % and 95 % of the answers (21.6 %): both of its
    outcomes are met."""
    data, offs = S.rolling(1, [1000] * 1500)
    plain = R.batch(data, offs, threads=16, seed_len=10, min_identity=0.95)
    sens = check(ctx, data, offs, seed_len=10, min_identity=0.95, sensitive=True)
    assert 0.05 < float((sens != plain).mean()) < 0.95


def test_random_records(ctx):
    data, offs = S.random_records(2, [1000] * 1500)
    for kw in ROLLING_SETTINGS + (dict(min_identity=0.95, sensitive=True),):
        exp = check(ctx, data, offs, seed_len=10, **kw)
        assert (exp == R.NONE).all()


def test_full_size_rolling(ctx):
    """1M x 1 kb, every record compared."""
    data, offs = S.rolling(3, [1000] * 1_000_000)
    exp = check(ctx, data, offs, seed_len=10, min_identity=0.95)
    assert 0.05 < float((exp != R.NONE).mean()) < 0.95
    check(ctx, data, offs, seed_len=10, max_mismatch=5, sensitive=True)


def test_mixed_lengths(ctx):
    rng = np.random.default_rng(4)
    lengths = np.exp(rng.uniform(np.log(200), np.log(20000), size=3000)).astype(np.int64)
    d1, o1 = S.rolling(5, lengths[:2000])
    d2, o2 = S.rolling(6, lengths[2000:], pmin=1000, pmax=6000, rate=0.003)
    data = np.concatenate([d1, d2])
    offs = np.concatenate([o1, o2[1:] + o1[-1]])
    for kw in (dict(min_identity=0.95), dict(min_identity=0.95, sensitive=True), dict(max_mismatch=5)):
        exp = check(ctx, data, offs, seed_len=10, **kw)
        assert 0.05 < float((exp != R.NONE).mean()) < 0.95


def test_tiny_records_between_long_ones(ctx):
    rng = random.Random(7)
    for k in (5, 10, 63):
        seqs = []
        for n in (0, 1, k, k + 1, 0, 2 * k, 1):
            seqs.append(S.periodic(rng, 5000, 1700, subs=3))
            seqs.append(S.periodic(rng, n, max(1, n // 2)))
        seqs.append(b"")
        for kw in (dict(min_identity=0.95), dict(max_mismatch=0, sensitive=True)):
            check_seqs(ctx, seqs, seed_len=k, **kw)


def test_long_records(ctx):
    """100 kb and 2 Mb, as a random monomer twice with a few substitutions and as plain random, and poly-A of 20 kb (cheap
    only because the scan is lazy).  The restatement's compared-byte count bounds the work of the batch."""
    rng = np.random.default_rng(8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    for n in (100_000, 2_000_000):
        mon = lut[rng.integers(0, 4, size=n // 2)]
        twice = np.concatenate([mon, mon])
        for p in rng.integers(0, n // 2 - 100, size=4):
            twice[p] = S.bump(int(twice[p]))
        seqs.append(twice.tobytes())
        seqs.append(lut[rng.integers(0, 4, size=n + 1)].tobytes())
    seqs.append(b"A" * 20000)
    data, offs = S.pack(seqs)
    for kw in (dict(min_identity=0.95), dict(min_identity=0.95, sensitive=True), dict(max_mismatch=3), dict(max_mismatch=4, sensitive=True)):
        exp, work = R.batch(data, offs, threads=16, want_work=True, seed_len=10, **kw)
        assert work < 10 ** 9
        compare(exp, ctx.monomerize_batch(data, offs, seed_len=10, **kw), kw, seqs)
        assert int(exp[0]) == 50_000 or kw == dict(max_mismatch=3)
        assert int(exp[2]) == 1_000_000 or kw == dict(max_mismatch=3)
        assert int(exp[4]) == 10


def test_device_views_at_every_shift(ctx):
    rng = random.Random(9)
    seqs = [S.periodic(rng, n, p, subs=1) for n, p in ((0, 1), (1, 1), (15, 5), (16, 8), (17, 4), (100, 33), (1030, 400), (2100, 1000), (31, 9))]
    data, offs = S.pack(seqs)
    for shift in range(16):
        for kw in (dict(seed_len=5, min_identity=0.9, sensitive=True), dict(seed_len=10, max_mismatch=1)):
            compare(R.batch(data, offs, **kw), device_batch(ctx, data, offs, shift=shift, **kw), kw, seqs)


def test_record_counts_round_a_workgroup(ctx):
    """A workgroup holds 4 waves = 4 records: counts on both sides of one and of several."""
    data, offs = S.rolling(10, [600] * 1100)
    kw = dict(seed_len=10, min_identity=0.95)
    exp = R.batch(data, offs, **kw)
    for n in (0, 1, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 1100):
        got = device_batch(ctx, data[:int(offs[n])], offs[:n + 1], **kw)
        compare(exp[:n], got, kw)


def test_back_to_back_batches_on_one_stream(ctx):
    """Batches with different settings enqueued without a wait in between: each keeps its own parameters."""
    import torch
    data, offs = S.rolling(11, [1000] * 800)
    d_bytes = torch.from_numpy(data).to(_dev())
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(_dev())
    runs = [dict(seed_len=10, min_identity=0.95), dict(seed_len=10, max_mismatch=0), dict(seed_len=5, min_identity=0.9, sensitive=True),
            dict(seed_len=63, max_mismatch=5), dict(seed_len=10, min_identity=0.95, sensitive=True)]
    outs = [torch.full((800,), SENTINEL, dtype=torch.int32, device=_dev()) for _ in runs]
    for kw, o in zip(runs, outs):
        ctx.monomerize_batch_device(d_bytes, d_offs, 800, o, **kw)
    ctx.synchronize()
    for kw, o in zip(runs, outs):
        compare(R.batch(data, offs, **kw), o.cpu().numpy().view(np.uint32), kw)


def test_bad_parameters_are_refused(ctx):
    import circkit_amd
    data, offs = S.pack([b"ACGTACGTACGTACGTACGTACGT"])
    for kw in (dict(seed_len=0), dict(seed_len=64), dict(seed_len=10, min_identity=-0.1), dict(seed_len=10, min_identity=1.5),
               dict(seed_len=10, min_identity=float("nan"))):
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.monomerize_batch(data, offs, **kw)
        assert e.value.code == -1, kw
        with pytest.raises(circkit_amd.CirckitError) as e:
            ctx.monomer_end_index(b"ACGTACGT", **kw)
        assert e.value.code == -1, kw
    with pytest.raises(ValueError, match="overlap_dist and overlap_min_identity"):
        ctx.monomerize_batch(data, offs, max_mismatch=1, min_identity=0.9)
    # identities at the ends of the range are fine, and the ctx still works after the refusals
    assert int(ctx.monomerize_batch(data, offs, seed_len=4, min_identity=1.0)[0]) == 4
    assert int(ctx.monomerize_batch(data, offs, seed_len=4, min_identity=0.0)[0]) == 4
    # a record of 2^32 symbols is refused before anything is read (the offsets alone say so)
    too_long = np.array([0, 2 ** 32], dtype=np.uint64)
    rc = ctx._lib.circkit_monomerize_batch(ctx._h, data.ctypes.data, too_long.ctypes.data, 1, ctypes.byref(circkit_amd.monomerize_params()),
                                           np.zeros(1, np.uint32).ctypes.data)
    assert rc == -4


def test_single_record_calls_on_the_known_answers(ctx):
    import circkit_amd
    from tests.test_monomerize_cpu import known_cases
    for name, seq, exp, kw in known_cases():
        e = ctx.monomer_end_index(seq, **kw)
        assert (seq if e is None else seq[:e]) == exp, (name, kw)
        assert e == R.end_index(seq, **kw)
    for name, seq, exp, kw in known_cases()[::7]:
        assert circkit_amd.monomerize(seq, **kw) == exp
    # any bytes, not only the normalized alphabet
    rng = random.Random(12)
    for _ in range(100):
        s = S.periodic(rng, rng.randint(0, 300), rng.randint(1, 90), bytes(range(256)), subs=rng.randint(0, 2))
        kw = dict(seed_len=rng.choice((1, 4, 10)), max_mismatch=rng.choice((0, 2)), sensitive=rng.random() < 0.5)
        assert ctx.monomer_end_index(s, **kw) == R.end_index(s, **kw)
    assert ctx.monomer_end_index(b"", seed_len=4) is None and circkit_amd.monomerize(b"") == b""
