"""GPU: circkit_orfs_batch / _device and circkit_find_orfs against the C restatement (tests/orfs_ref.c)."""
import json
import os
import random

import numpy as np
import pytest

from tests import orfs_ref as R
from tests.test_orfs_cpu import GRID_CODONS, _pack, adversarial_batch, known_answers, random_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import circkit_amd
    c = circkit_amd.Context(0)
    yield c
    c.close()


def check(ctx, seqs, **kw):
    d, o = _pack(seqs)
    eo, e = R.orfs_batch(d, o, threads=16, **kw)
    api_kw = dict(kw)
    api_kw["strands"] = api_kw.get("strands", 3)
    api_kw["mode"] = api_kw.get("mode", 0)
    got = ctx.orfs_batch(d, o, **api_kw)
    assert np.array_equal(got["offsets"], eo), kw
    for f in ("start", "stop", "length", "wraps", "strand"):
        assert np.array_equal(got[f], e[f]), (f, kw)
    return len(e)


def test_find_orfs_known_answers(ctx):
    for case in known_answers():
        if case["call"] == "longest":
            d, o = _pack([case["seq"].encode()])
            g = ctx.orfs_batch(d, o, strands="forward", mode="longest")
            got = [(int(g["start"][k]), int(g["stop"][k]), int(g["wraps"][k]), int(g["length"][k])) for k in range(len(g["start"]))]
        else:
            got = ctx.find_orfs(case["seq"].encode())
        assert got == [tuple(e) for e in case["expected"]], case["name"]


def test_find_orfs_matches_restatement(ctx):
    rng = random.Random(11)
    for _ in range(200):
        s = bytes(rng.choice(b"ATGCa") for _ in range(rng.randint(0, 200)))
        assert ctx.find_orfs(s) == (R.find_orfs(s) if len(s) >= 2 else []), s


def test_every_length_mod_three(ctx):
    rng = random.Random(1)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(L)) for L in range(2, 3001)]
    for mode in (0, 1):
        assert check(ctx, seqs, mode=mode) > 0


def test_adversarial_parameter_grid(ctx):
    rng = random.Random(2)
    for _ in range(120):
        check(ctx, adversarial_batch(rng, 60), **random_params(rng))


def test_full_grid_on_one_batch(ctx):
    rng = random.Random(3)
    seqs = adversarial_batch(rng, 200)
    seqs += [b"ATG" + b"C" * 997, b"CCAT" + b"G" * 500, b"ATGNNN-TAA" * 20, b"atgaaataa" * 10, b"ATG" * 300]
    for st, sp in GRID_CODONS[:3]:
        for min_length in (0, 75, 10 ** 12):
            for min_wraps in range(4):
                for max_wraps in range(4):
                    for req in (False, True):
                        for ratio in (0, 0.5, 1, 1.5):
                            if rng.random() < 0.85:
                                continue              # a random eighth of the grid per codon set, every value covered
                            for strands in (1, 2, 3):
                                for mode in (0, 1):
                                    check(ctx, seqs, start_codons=st, stop_codons=sp, min_length=min_length, min_wraps=min_wraps,
                                          max_wraps=max_wraps, require_stop=req, min_ratio=ratio, strands=strands, mode=mode)


def test_long_records(ctx):
    rng = random.Random(4)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(100_000)),
            bytes(rng.choice(b"ACGT") for _ in range(2_000_001)),
            b"ATG" + b"C" * 99_998,                                   # no stop anywhere
            bytes(rng.choice(b"ACG") for _ in range(2_000_000)),     # no T: starts only, no stop
            (b"ATGATGTAA" * 22_223)[:200_002]]                      # an ORF per 9 symbols (the heapsort path)
    for mode in (0, 1):
        check(ctx, seqs, mode=mode)
        check(ctx, seqs, mode=mode, min_length=0, require_stop=False, max_wraps=3)


def test_1m_records_of_1kb_in_full(ctx):
    import circkit_amd
    n, L = 1_000_000, 1000
    from oracle import oracle as O
    d = O.synth_fill(5, 0, n * L)
    o = np.arange(n + 1, dtype=np.uint64) * L
    eo, e = R.orfs_batch(d, o, threads=16, min_length=75, require_stop=True)
    got = ctx.orfs_batch(d, o, min_length=75, require_stop=True)
    assert np.array_equal(got["offsets"], eo)
    for f in ("start", "stop", "length", "wraps", "strand"):
        assert np.array_equal(got[f], e[f]), f
    assert len(e) > n


def test_device_batch_capacity_overflow(ctx):
    import torch
    import circkit_amd
    rng = random.Random(6)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(2, 3000))) for _ in range(3000)]
    d, o = _pack(seqs)
    eo, e = R.orfs_batch(d, o, threads=16)
    total = int(eo[-1])
    dev = torch.device("cuda", 0)
    db, do = torch.from_numpy(d.copy()).to(dev), torch.from_numpy(o.astype(np.int64)).to(dev)
    doff = torch.zeros(len(seqs) + 1, dtype=torch.int64, device=dev)
    small = torch.zeros((total - 1) * 24, dtype=torch.uint8, device=dev)
    ctx.orfs_batch_device(db, do, len(seqs), doff, small, total - 1)
    with pytest.raises(circkit_amd.CirckitError) as ex:
        ctx.orfs_status()
    assert ex.value.code == -5 and str(total) in str(ex.value)
    assert np.array_equal(doff.cpu().numpy().astype(np.uint64), eo)
    big = torch.zeros(total * 24, dtype=torch.uint8, device=dev)
    ctx.orfs_batch_device(db, do, len(seqs), doff, big, total)
    assert ctx.orfs_status() == total
    got = big.cpu().numpy().view(circkit_amd.api.ORF_DTYPE)
    assert np.array_equal(got, e)
    # the host form reports the total and succeeds when called again (Context.orfs_batch grows from a small guess)
    res = ctx.orfs_batch(d, o)
    assert np.array_equal(res["start"], e["start"])
