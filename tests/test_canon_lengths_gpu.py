"""Every record length through every build of the canonicalize kernels, on the device (run with -m gpu).

The lane constants of canon_pair.h, canon_fast.h, canon_stream.h and canon_mixed.h are functions of the record's length, of
n mod 16 and of the record's place in its 16-byte chunk, and launch_canon picks among a dozen builds by the batch's mode and the
outputs asked for.  The emulator tests prove the algorithm for every length; what hipcc made of it for gfx950 was checked at
random lengths only.  Here tests/length_sets.py's sweeps -- one record of every length per route, in two orders -- and the
emulator's crafted sets go through circkit_canonicalize_batch_device / circkit_lmsr_batch_device on one ctx, the device deciding
the mode: every record of every output against the oracle, canaries round every buffer (tests/test_gpu_outputs.py's Batch), the
reported mode against length_sets.expected_mode, each call three times in a row (a wrong mode guess first, a settled one last),
the bytes + hash call at all sixteen payload alignments, and once more in a child process in which no batch guesses its mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import length_sets as LS           # noqa: E402
from tests import seqsets                     # noqa: E402
from tests.test_gpu_outputs import PAD, Batch  # noqa: E402

pytestmark = pytest.mark.gpu

# routes in an order that changes the mode (1 / 2 / 3, MODE_ALPHA, MODE_SHORT) at every step: the first call of a set runs on the
# builds the previous set's mode chose
ROUTE_ORDER = ["stream_bytes", "mixed", "pair_bytes", "two_word", "stream_n", "mixed_n", "pair_hash", "two_word_hash", "aux_one_word"]
CRAFTED_ORDER = ["n_mask_1", "mixed_batch", "pair_two_records_14", "mixed_batch_n", "pair_every_length", "mixed_prefix_rule", "n_mask_3",
                 "mixed_tied_key", "pair_two_records_15", "mixed_seen_twice_n", "hash_only_views", "mixed_seen_twice", "mixed_palindrome",
                 "mixed_n_in_window", "mixed_fused_xxh3", "mixed_fused_xxh3_n"]
assert sorted(ROUTE_ORDER) == sorted(LS.ROUTES) and sorted(CRAFTED_ORDER) == sorted(LS.CRAFTED)


def cells(route):
    """the route's calls: (outputs, lmsr)"""
    r = LS.ROUTES[route]
    return [(o, False) for o in r["outs"]] + [(o, True) for o in r["lmsr"]]


N_PASSES = max(len(cells(r)) for r in LS.ROUTES)


class Sets:
    """The sets as device batches (built once, kept unchanged), and one checked call of one of them."""

    def __init__(self, ctx, dev, O):
        self.ctx, self.dev, self.O, self.batches = ctx, dev, O, {}

    def batch(self, key):
        if key not in self.batches:
            seqs = LS.sweep(key[1], key[2])[0] if key[0] == "sweep" else LS.CRAFTED[key[1]][0]()
            B = Batch(seqs, self.dev, self.O, lmsr_oracle=key[0] == "sweep" and bool(LS.ROUTES[key[1]]["lmsr"]))
            B.lens = [len(s) for s in seqs]
            self.batches[key] = B
        return self.batches[key]

    def call(self, key, outs, lmsr, layout, what):
        B = self.batch(key)
        want = LS.expected_mode(B.lens, B.data, B.offs, "h" in outs, lmsr or "i" in outs or "s" in outs) & 3
        got = B.run(self.ctx, outs, layout, lmsr=lmsr)
        assert got["status"] == 0, "%s: %d records nothing could take" % (what, got["status"])
        assert got["mode"] == want, "%s: mode %d, expected %d" % (what, got["mode"], want)
        B.check(got, outs, lmsr=lmsr, what=what)                       # (names the output, the records and their lengths)

    def three_times(self, key, outs, lmsr, reps=3):
        """the same call three times in a row: plain layout, offsets[0] = 24 at an odd address, plain"""
        for rep in range(reps):
            self.call(key, outs, lmsr, rep == 1, "%s/%s%s/rep%d" % ("/".join(key[1:]), "lmsr " if lmsr else "", outs, rep))

    def at_shift(self, key, outs, shift, lead):
        """one call with the payload and output pointers `shift` bytes off a 64-byte boundary and offsets[0] = lead"""
        import torch
        B = self.batch(key)
        raw = np.full(PAD + shift + lead + B.nb + PAD, 0xC3, dtype=np.uint8)
        raw[PAD + shift + lead:PAD + shift + lead + B.nb] = B.data
        d_raw = torch.from_numpy(raw).to(self.dev)
        d_off = torch.from_numpy((B.offs + np.uint64(lead)).astype(np.int64)).to(self.dev)
        B.layouts.append(dict(shift=shift, lead=lead, d_raw=d_raw, d_raw0=d_raw.clone(), d_off=d_off, d_off0=d_off.clone(),
                              d_out_raw=torch.empty_like(d_raw)))
        try:
            self.call(key, outs, False, len(B.layouts) - 1, "%s/%s/shift %d lead %d" % ("/".join(key[1:]), outs, shift, lead))
        finally:
            B.layouts.pop()


@pytest.fixture(scope="module")
def sets():
    import torch
    import circkit_amd
    from oracle import oracle
    oracle.lib()
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield Sets(ctx, torch.device("cuda", 0), oracle)
    ctx.close()


@pytest.mark.parametrize("k", range(N_PASSES))
@pytest.mark.parametrize("order", LS.ORDERS)
def test_every_length_on_every_route(sets, order, k):
    """Pass k: the k-th output set of every route (length_sets.ROUTES: bytes, bytes + hash, hash alone; bytes + index + strand and
    lmsr for the index builds), the routes in an order that changes the mode at every step, each call three times."""
    for route in ROUTE_ORDER:
        c = cells(route)
        if k < len(c):
            sets.three_times(("sweep", route, order), c[k][0], c[k][1])


@pytest.mark.parametrize("route", ROUTE_ORDER)
@pytest.mark.parametrize("order", LS.ORDERS)
def test_every_length_at_every_payload_alignment(sets, order, route):
    """bytes + XXH3 of every sweep with the payload at all sixteen alignments (offsets[0] = 0 at the even shifts, 24 at the odd
    ones): the record's place in its chunk moves with the pointer, the aligned-chunk loads of every build with it."""
    for shift in range(16):
        sets.at_shift(("sweep", route, order), "bh", shift, 24 * (shift & 1))


@pytest.mark.parametrize("name", CRAFTED_ORDER)
def test_crafted_sets_on_the_device(sets, name):
    """The emulator tests' crafted sets (prefix rule, extension edges, ties, palindromes, the winner seen twice by one lane, N inside
    the minimal window, XXH3 block and stripe edges, the pair build's partners) in batches of the mode their emulator test aims at."""
    _, aim, outs = LS.CRAFTED[name]
    B = sets.batch(("crafted", name))
    for o in outs:
        assert LS.crafted_mode_matches(aim, LS.expected_mode(B.lens, B.data, B.offs, "h" in o, False), o)
        sets.three_times(("crafted", name), o, False)


def _no_guess_pass(sets):
    """bytes and bytes + hash of every sweep and crafted set (two calls each), for the child process"""
    keys = [("sweep", r, o) for o in LS.ORDERS for r in ROUTE_ORDER] + [("crafted", n) for n in CRAFTED_ORDER]
    for key in keys:
        for outs in ("b", "bh"):
            sets.three_times(key, outs, False, reps=2)
    return len(keys)


def test_every_build_launched_for_every_batch():
    """CIRCKIT_NO_MODE_GUESS=1 (read once per process: a fresh child): no batch runs on a guessed mode, every batch launches all
    builds and the ones its own mode does not name must return without a trace -- bytes and bytes + hash of every set."""
    env = dict(os.environ, CIRCKIT_NO_MODE_GUESS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0 and "NO-GUESS-OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


if __name__ == "__main__":
    import torch
    import circkit_amd
    from oracle import oracle
    assert os.environ.get("CIRCKIT_NO_MODE_GUESS")
    oracle.lib()
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = _no_guess_pass(Sets(ctx, torch.device("cuda", 0), oracle))
    ctx.close()
    print("NO-GUESS-OK %d sets" % n)
