"""The monomerize wave routine (circkit_amd/csrc/monomerize.h) run as 64 fibers per wave on the CPU (tests/emu/mono_emu.cpp:
UBSan + bounds checks, a lane that skips a collective deadlocks and is reported) against the restatement (tests/mono_ref.c).
Every record of every set is compared; the loader checks canaries round the output array and that the input is unchanged."""
import random

import numpy as np
import pytest

from tests import mono_ref as R
from tests import mono_sets as S
from tests.emu import mono_emu as E


def check(seqs, base_shift=0, lead=0, **kw):
    data, offs = S.pack(seqs)
    exp = R.batch(data, offs, threads=4, **kw)
    got = E.monomerize_batch(data, offs, base_shift=base_shift, lead=lead, **kw)
    bad = np.nonzero(exp != got)[0]
    assert len(bad) == 0, (kw, int(bad[0]), len(seqs[bad[0]]), seqs[bad[0]][:80], int(exp[bad[0]]), int(got[bad[0]]))
    return exp


@pytest.mark.parametrize("k", (1, 5, 10, 63))
def test_every_length(k):
    """Every length 0..300 (n <= k, n = k + 1, n = 2k - 1, n = 2k among them), every cut-off, plain and sensitive."""
    seqs = S.every_length(random.Random(100 + k))
    seqs += [b"A" * n for n in (k - 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1)]
    some = 0
    for kw in S.settings((k,)):
        some += int((check(seqs, **kw) != R.NONE).sum())
    assert some > 1000


@pytest.mark.parametrize("k", (5, 10, 63))
def test_adversarial(k):
    seqs = S.adversarial()
    for kw in S.settings((k,)):
        check(seqs, **kw)


def test_adversarial_seed_1():
    """With a seed of one symbol nearly every position is an occurrence: the records of up to 700 bytes of the set, and the
    longer ones under the two cut-offs that end a candidate at once."""
    seqs = S.adversarial()
    short = [s for s in seqs if len(s) <= 700]
    assert len(short) >= 30
    for kw in S.settings((1,)):
        check(short, **kw)
    for kw in (dict(max_mismatch=0), dict(min_identity=1.0)):
        for sv in (False, True):
            check(seqs, seed_len=1, sensitive=sv, **kw)


def test_identity_boundaries():
    for rec, ident, ovl, nm, accepted in S.identity_boundaries():
        for sv in (False, True):
            exp = check([rec], seed_len=5, min_identity=ident, sensitive=sv)
            if not sv:
                assert int(exp[0]) == (ovl if accepted else R.NONE)


def test_known_answers():
    from tests.test_monomerize_cpu import known_cases
    for name, seq, exp, kw in known_cases():
        if name == "ambivirus" and (kw["seed_len"] not in (10, 63) or kw["max_mismatch"] not in (0, 10)):
            continue                      # the 5 kb genome: the corners of its grid here, the whole grid on the GPU
        got = check([seq], **kw)
        assert seq[:len(seq) if int(got[0]) == R.NONE else int(got[0])] == exp


def test_every_alignment_and_position_in_the_batch():
    """The payload pointer at every shift mod 16, canary bytes in front of the first record."""
    rng = random.Random(8)
    seqs = [S.periodic(rng, n, p, subs=1) for n, p in ((0, 1), (1, 1), (15, 5), (16, 8), (17, 4), (100, 33), (1030, 400), (2100, 1000))]
    for shift in range(16):
        check(seqs, base_shift=shift, lead=(shift * 7) % 23, seed_len=5, min_identity=0.9, sensitive=True)
        check(seqs, base_shift=shift, lead=shift, seed_len=10, max_mismatch=1)
