"""Every admission boundary of the LDS stages, their teams, the mixed-length kernels, the global scratch and the single-record
launch, on the device (run with -m gpu).

tests/tier_sets.py derives the boundary lengths from the restated predicates and capacities and builds records whose class fixes
the governing predicate; tests/test_tier_sets_cpu.py proves the arithmetic and the LDS footprints on the emulator for stages A, C
and the mixed builds.  Only the device runs the sixteen-wave team stage, the global-scratch kernel, the idle / busy builds of
canon_kernel<4> and canon_kernel<1> with its five slice sizes.  Here: runs of four boundary records of one length (the four waves
of a workgroup hold maximal records at the same time: an overrun lands in a live neighbour), each followed by four short records
that need the workgroup's decode tables, every record of every output against the oracle, canaries round every device buffer
(tests/test_gpu_outputs.py's Batch).

The pure pair at the default scratch's phase-1 edge (16 777 184 / 5 symbols) is in: making the two records takes 0.5 s and the
oracle 0.5 s (16 threads) on the build machine's CPU."""
import ctypes

import numpy as np
import pytest

from tests import length_sets as LS
from tests import seqsets
from tests import tier_sets as T
from tests.test_gpu_outputs import S_BYTE, S_HASH, S_IDX, S_STRAND, Batch

pytestmark = pytest.mark.gpu

CIRCKIT_ERR_TOO_LONG = -4


class Env:
    def __init__(self, ctx, dev, O):
        self.ctx, self.dev, self.O, self.batches = ctx, dev, O, {}

    def batch(self, key, build):
        """a record set as a device batch with its oracle results: built once, kept unchanged"""
        if key not in self.batches:
            seqs = build()
            B = Batch(seqs, self.dev, self.O, lmsr_oracle=False)
            B.lens = [len(s) for s in seqs]
            self.batches[key] = B
        return self.batches[key]

    def checked(self, B, outs, what, layout=0, want_mode=3):
        got = B.run(self.ctx, outs, layout)
        assert got["status"] == 0, "%s: %d records nothing could take" % (what, got["status"])
        if want_mode is not None:
            assert got["mode"] == want_mode, "%s: mode %d, expected %d" % (what, got["mode"], want_mode)
        B.check(got, outs, what=what)


@pytest.fixture(scope="module")
def env():
    import torch
    import circkit_amd
    from oracle import oracle
    oracle.lib()
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    yield Env(ctx, torch.device("cuda", 0), oracle)
    ctx.close()


def _stage(env, stage, order):
    B = env.batch(("stage", stage, order), lambda: T.stage_batch(stage, order)[0])
    for want_hash, aux in ((False, False), (True, False), (True, True)):
        assert LS.expected_mode(B.lens, B.data, B.offs, want_hash, aux) & 3 == 3
    return B


def _idle_maker(env):
    """all records of 1 kb: the LDS stages find nothing, the next batch's launch uses canon_kernel<4, false> and the small grids"""
    return env.batch(("idle",), lambda: [seqsets._np_seq(np.random.default_rng(5), 1000) for _ in range(600)])


@pytest.mark.parametrize("order", T.ORDERS)
@pytest.mark.parametrize("stage", ["A", "C", "T"])
def test_stage_chain_host_api_all_outputs(env, stage, order):
    """circkit_canonicalize_batch (the host sees the offsets and picks mode 3) with bytes, index, strand and XXH3 -- the index
    builds in front, then canon_kernel<4> for stages A and C and the team stage -- of every reachable triple's six probe lengths."""
    B = _stage(env, stage, order)
    got = env.ctx.canonicalize_batch(B.data, B.offs, want_bytes=True, want_index=True, want_strand=True, want_xxh3=True)
    assert env.ctx.batch_status() == 0
    assert env.ctx.last_batch_mode() == 3
    exp_b, exp_h, exp_i, exp_s = B.exp
    for name, exp in (("bytes", exp_b), ("index", exp_i), ("strand", exp_s), ("xxh3", exp_h)):
        if not np.array_equal(got[name], exp):
            if name == "bytes":
                bad = [k for k in range(B.n) if not np.array_equal(got[name][B.offs[k]:B.offs[k + 1]], exp[B.offs[k]:B.offs[k + 1]])]
            else:
                bad = np.nonzero(got[name] != exp)[0].tolist()
            tags = T.stage_batch(stage, order)[1]
            raise AssertionError("%s/%s %s: %d records differ, first %s" % (stage, order, name, len(bad), [(k, tags[k]) for k in bad[:6]]))


@pytest.mark.parametrize("outs", ["b", "bish", "h"])
@pytest.mark.parametrize("stage", ["A", "C", "T"])
def test_stage_chain_device_api_idle_then_busy_builds(env, stage, outs):
    """Bytes only (the mixed-length kernel in front, lean admission), bytes + index + strand + XXH3 (the index builds in front) and
    the hash alone (views; Batch.check compares with XXH3 of the oracle's canonical bytes): an all-1 kb batch first, so that the
    boundary batch runs on the idle builds (canon_kernel<4, false>: no 4-bit team, small grids), then the boundary batch again on
    the busy builds with the 4-bit team.  All three results are checked."""
    B = _stage(env, stage, "reversed" if outs == "bish" else "as_built")
    idle = _idle_maker(env)
    env.checked(idle, outs, "idle/" + outs, want_mode=1)
    env.checked(idle, outs, "idle again/" + outs, want_mode=1)       # (the first may itself have followed a busy batch)
    env.checked(B, outs, "%s/%s on the idle builds" % (stage, outs))
    env.checked(B, outs, "%s/%s on the busy builds" % (stage, outs), layout=1)


def _mixed_batch(n_build):
    """the six probe lengths of every triple of the mixed-length kernel's pure / N build, each behind a filler record whose length
    shifts the next record's alignment (N build: with N among its first symbols, which is what makes the batch MODE_ALPHA)"""
    rng = np.random.default_rng(31)
    seqs = []
    for ti, t in enumerate(T.TRIPLES):
        if t.stage == ("mixed_n" if n_build else "mixed"):
            for k, L in enumerate(T.probes(T.triple_n_max(t))):
                fill = seqsets._np_seq(rng, 2100 + int(rng.integers(0, 16)))
                seqs += [LS._with_n(rng, fill) if n_build else fill, T.make(t.cls, L, 500 + ti + k)]
    return seqs + [seqsets._np_seq(rng, 2100)]


@pytest.mark.parametrize("n_build", [False, True])
def test_mixed_kernel_boundaries_at_all_sixteen_payload_shifts(env, n_build):
    """Bytes only and bytes + XXH3 through the mixed-length kernel (pure build: the pure classes; N build: with and without N, the
    filler with N) with the payload at all sixteen alignments: the alignment enters LeanGeom, and lean_strand_dw is sized for
    the worst shift."""
    import torch
    want = [t for t in T.TRIPLES if t.stage == ("mixed_n" if n_build else "mixed")]
    B = env.batch(("mixed", n_build), lambda: _mixed_batch(n_build))
    assert {len(s) for s in B.seqs} >= {T.triple_n_max(t) + d for t in want for d in (0, 1)}
    assert bool(LS.expected_mode(B.lens, B.data, B.offs, False, False) & LS.MODE_ALPHA) == n_build
    from tests.test_gpu_outputs import PAD
    for shift in range(16):
        lead = 24 * (shift & 1)
        raw = np.full(PAD + shift + lead + B.nb + PAD, 0xC3, dtype=np.uint8)
        raw[PAD + shift + lead:PAD + shift + lead + B.nb] = B.data
        d_raw = torch.from_numpy(raw).to(env.dev)
        d_off = torch.from_numpy((B.offs + np.uint64(lead)).astype(np.int64)).to(env.dev)
        B.layouts.append(dict(shift=shift, lead=lead, d_raw=d_raw, d_raw0=d_raw.clone(), d_off=d_off, d_off0=d_off.clone(),
                              d_out_raw=torch.empty_like(d_raw)))
        try:
            for outs in ("b", "bh"):
                env.checked(B, outs, "mixed%s/%s/shift %d" % ("_n" if n_build else "", outs, shift), layout=len(B.layouts) - 1)
        finally:
            B.layouts.pop()


def _edge_pairs(cap, seed):
    """(class, predicate) -> the records of n_max and n_max + 1 against `cap` dwords: the team's three predicates and wave 0's two"""
    out = []
    for k, (cls, pred) in enumerate((("pure", "strand2"), ("few_n", "2n"), ("gap", "strand4"), ("byte", "need8"), ("tie", "need2"),
                                     ("pure_rc", "strand2"), ("few_n_rc", "2n"))):
        nm = T.n_max(pred, cap)
        out.append((cls, pred, T.make(cls, nm, seed + k), T.make(cls, nm + 1, seed + 10 + k)))
    return out


def test_team_stage_edges_go_on_to_the_global_scratch(env):
    """The last admitted and the first refused length of the sixteen-wave team stage (16 x 2511 = 40176 dwords, not 40188) for the
    team's three predicates and wave 0's two, between ordinary records: the + 1 records come back right from the global-scratch
    kernel.  Device API with every output, then the host API."""
    def build():
        seqs = seqsets.random_mixed(61, 12, 200, 20000)
        for cls, pred, a, b in _edge_pairs(T.TEAM_WAVES * T.TEAM_SLICE_DW, 70):
            seqs += [a, b] + seqsets.random_mixed(62 + len(seqs), 3, 500, 30000, b"ACGTN")
        return seqs
    B = env.batch(("team edges",), build)
    for cls, pred, a, b in _edge_pairs(T.TEAM_WAVES * T.TEAM_SLICE_DW, 70):
        T.check_class(cls, a)
        T.check_class(cls, b)
        assert T.PREDICATES[pred](len(a)) <= 40176 < T.PREDICATES[pred](len(b))
    for outs in ("bish", "b", "h"):
        env.checked(B, outs, "team edges/" + outs)
    got = env.ctx.canonicalize_batch(B.data, B.offs, want_bytes=True, want_index=True, want_strand=True, want_xxh3=True)
    assert env.ctx.batch_status() == 0
    for name, exp in zip(("bytes", "xxh3", "index", "strand"), B.exp):
        assert np.array_equal(got[name], exp), name


@pytest.mark.parametrize("cls,pred", [("byte", "need8"), ("gap", "strand4"), ("pure", "strand2")])
def test_phase_one_edge_of_the_default_scratch(env, cls, pred):
    """Phase 1 of the global-scratch kernel gives a workgroup 2^20 dwords, phase 2 the whole scratch (256 MiB): the byte pair, the
    4-bit pair and the pure pair at the phase-1 edge -- n_max done in phase 1, n_max + 1 passed on to phase 2 and done there."""
    nm = T.n_max(pred, T.GSLICE1_DW)
    assert T.PREDICATES[pred](nm) <= 1 << 20 < T.PREDICATES[pred](nm + 1)
    B = env.batch(("phase 1 edge", cls), lambda: seqsets.random_mixed(81, 6, 200, 5000) + [T.make(cls, nm, 90), seqsets._np_seq(np.random.default_rng(3), 3000),
                                                                                         T.make(cls, nm + 1, 95)])
    for outs in ("bish", "h"):
        env.checked(B, outs, "phase 1 edge %s/%s" % (cls, outs))
    del env.batches[("phase 1 edge", cls)]                  # (tens of MB on the device: not kept)


def test_host_batch_on_a_fresh_ctx_leaves_the_device_entry_points_their_default_scratch(env):
    """Found by the test above: the host API sized a fresh ctx's scratch for its own longest record (here 100 kb: 213 KB), and
    launch_canon allocates the 256 MiB default only when there is no scratch at all -- every later device batch then had records
    beyond ~50 k dwords refused (CIRCKIT_ERR_TOO_LONG) although include/circkit.h promises them the default.  A host batch with one
    record beyond the LDS stages on a new ctx, then a device batch with byte records of 0.4 and 2 M symbols."""
    import torch
    import circkit_amd
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        first = [T.make("byte", 100000, 1)] + seqsets.random_mixed(5, 4, 100, 3000)
        data, offs = seqsets.pack(first)
        assert T.worst_case_dw(100000) > T.TIER_DW[4]
        got = ctx.canonicalize_batch(data, offs, want_bytes=True)
        assert ctx.batch_status() == 0 and np.array_equal(got["bytes"], env.O.canonicalize_batch(data, offs, True, False, threads=4)[0])
        B = env.batch(("behind a host batch",), lambda: seqsets.random_mixed(6, 4, 100, 3000) + [T.make("byte", 400000, 2), T.make("byte", 2000000, 3)])
        Env(ctx, env.dev, env.O).checked(B, "bish", "device batch behind a fresh ctx's host batch", want_mode=None)
    finally:
        ctx.close()


SMALL_SCRATCH = 1 << 20                      # bytes: phase 1 and phase 2 are then one slice of 262 144 dwords


@pytest.fixture(scope="module")
def small(env):
    """a second ctx whose long-record scratch is the smallest there is, set before its first batch (the scratch only grows)"""
    import torch
    import circkit_amd
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_long_record_scratch(SMALL_SCRATCH)
    yield Env(ctx, env.dev, env.O)
    ctx.close()


def test_scratch_edges_without_large_records(env, small):
    """With a 1 MiB scratch every class's n_max record (against 262 144 dwords) completes; its n_max + 1 record is left untouched
    and counted by circkit_ctx_batch_status, which returns CIRCKIT_ERR_TOO_LONG; every other record of the batch is still right;
    in the hash-only form the refused record's view is 0, i.e. its hash slot holds XXH3 of the record as it is."""
    cap = SMALL_SCRATCH // 4
    pairs = _edge_pairs(cap, 170)
    fill = seqsets.random_mixed(171, 10, 200, 20000, b"ACGTN")
    ok = env.batch(("scratch ok",), lambda: fill[:5] + [a for _, _, a, _ in pairs] + fill[5:])
    for outs in ("bish", "h", "b"):
        small.checked(ok, outs, "1 MiB scratch, every n_max/" + outs)
    seqs = fill[:3]
    refused = []
    for _, _, a, b in pairs:
        refused.append(len(seqs) + 1)
        seqs += [a, b, fill[len(refused)]]
    B = env.batch(("scratch refused",), lambda: seqs)
    n_un = ctypes.c_uint32(0)
    for outs in ("bis", "h", "b"):
        got = B.run(small.ctx, outs, 0)
        assert got["status"] == len(refused), (outs, got["status"])
        assert small.ctx._lib.circkit_ctx_batch_status(small.ctx._h, ctypes.byref(n_un)) == CIRCKIT_ERR_TOO_LONG and n_un.value == len(refused)
        exp_b, exp_h, exp_i, exp_s = B.exp
        for k in range(B.n):
            lo, hi = int(B.offs[k]), int(B.offs[k + 1])
            what = "record %d (%d symbols) / %s" % (k, hi - lo, outs)
            if k in refused:
                assert (got["b"][lo:hi] == S_BYTE).all() and got["i"][k] == S_IDX and got["s"][k] == S_STRAND, what + ": refused, but written"
                if outs == "h":
                    assert got["h"][k] == env.O.xxh3_64(B.seqs[k]), what + ": the refused record's view is not 0"
                continue
            if "b" in outs:
                assert np.array_equal(got["b"][lo:hi], exp_b[lo:hi]), what
            if "i" in outs:
                assert got["i"][k] == exp_i[k] and got["s"][k] == exp_s[k], what
            if "h" in outs:
                assert got["h"][k] == exp_h[k], what
        if "h" not in outs:
            assert (got["h"] == S_HASH).all()
    small.checked(ok, "bish", "behind a batch with refused records")


@pytest.mark.parametrize("cls", T.SINGLE_CLASSES)
def test_single_record_calls_at_every_tier_switch(env, cls):
    """circkit_canonicalize / circkit_lmsr / circkit_lmsr_index at launch_single's four tier switches (worst_case_dw against
    1280 / 1900 / 3324 / 9980 dwords) and where the single launch hands over to the batch pipeline: canon_kernel<1> with each of
    its five slice sizes; in the tie and byte classes the big slices get real work."""
    switches, handover = T.single_switches()
    assert all(T.worst_case_dw(n) <= c < T.worst_case_dw(n + 1) for n, c in zip(switches, T.TIER_DW)) and handover > switches[-1]
    assert T.worst_case_dw(handover) <= T.TIER_DW[4]              # (canon_global_one_kernel is never needed)
    for k, L in enumerate([n + d for n in switches + [handover] for d in (0, 1)]):
        s = T.make(cls, L, 300 + k)
        T.check_class(cls, s)
        exp_b, _, _ = seqsets.expected(env.O, s)
        assert env.ctx.canonicalize(s) == exp_b, "canonicalize %s %d" % (cls, L)
        assert env.ctx.lmsr(s) == env.O.lmsr(s), "lmsr %s %d" % (cls, L)
        assert env.ctx.lmsr_index(s) == env.O.lmsr_index(s), "lmsr_index %s %d" % (cls, L)
