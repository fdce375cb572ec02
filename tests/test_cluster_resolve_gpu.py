"""GPU: circkit_cluster_candidates_device on every route of the uniq resolve it runs over its band keys, and the ctx's uniq table
between the cluster unit and the uniq unit.  The sets are tests/cluster_route_sets.py's (tests/test_cluster_route_sets_cpu.py
establishes the route of each on the CPU); every offset, pair and total is exact against the array yardstick tests/cluster_np.py,
which tests/test_cluster_np_cpu.py holds against the definition.  Canaries and the row check are tests/test_cluster_gpu.py's.

  (a) every set: direct below 2^19 keys, buckets that stay in LDS (64, 63 and 5 bands), buckets with the HBM fallback behind
      them (a flood of NO_KEY keys in the last bucket; 64 keys of 8192 rows each), direct beyond 2600 * 8192 keys
  (b) the routes one after the other on one ctx: no flag, table size or scratch of one reaches the next
  (c) lds_first with CIRCKIT_UNIQ_NO_BUCKETS=1 in a child process: the same pairs
  (d) circkit_cluster_batch at a bucketed size on short records, nearly all of whose keys are NO_KEY
  (e) the uniq table belongs to whoever used it last: a streaming uniq before, an overflow before, an overflow between a
      candidates call and its status (the status answers for its own resolve), circkit_uniq_first_seen behind

Wall time of this file on one MI355X: 14 tests in about 7 s (1.7 s of it the first ctx, 2.7 s the child of (c), 0.9 s the 21 M keys
of beyond_buckets, 0.7 s of that the yardstick).

What the file was seen to catch, on scratch builds of the library with one change each (both in bounds):
  circkit_cluster.hip as before the status kept its own overflow count   the overflow-between test alone fails: (OOM, 7) for (OK, 7)
  `(uint32_t)fp / E.n_bands` -> `>> 6` in write_wave                     lds_63 and lds_5x3 fail on their pairs; the 64-band sets pass"""
import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import cluster_np as N
from tests import cluster_ref as C
from tests import cluster_route_sets as RS
from tests import cluster_sets as S
from tests import sketch_ref as R
from tests import sketch_sets as SS
from tests import test_cluster_gpu as G
from tests import uniq_keys as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG, OOM = 0, -1, -5
BASE = 7_000_000_000
LOOKUP_CANARY = 0x5A5A5A5A5A5A5A5A


@pytest.fixture
def ctx():
    import circkit_amd
    import torch
    assert "CIRCKIT_UNIQ_NO_BUCKETS" not in os.environ, "with it no call here takes the bucketed route"
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def run_set(ctx, name):
    """One candidates call over a set at the capacity that always suffices: (offsets, pairs buffer), after the canary and row
    checks, the status (OK, total) and the comparison with the yardstick."""
    rows, nb, bb = RS.rows_of(name)
    exp_off, exp_pairs = RS.expected(name)
    c = G.Candidates(rows.copy(), len(rows) * nb)              # (the set's rows are read-only and stay the set's)
    c.launch(ctx, nb, bb)
    rc, total = G.candidates_status(ctx)
    off, pairs = c.result()
    assert (rc, total) == (OK, len(exp_pairs)), (name, rc, total, len(exp_pairs))
    assert np.array_equal(off, exp_off), name
    assert np.array_equal(pairs[:total], exp_pairs), name
    assert (pairs[total:] == G.PAIR_CANARY).all(), name
    return off, pairs


# ---- (a) every set ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in RS.SETS if n != "beyond_buckets"])
def test_every_route(ctx, name):
    first = run_set(ctx, name)
    if name == "lds_first":                                  # again on the same ctx: bit-identical, and the yardstick's both times
        second = run_set(ctx, name)
        assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


def test_beyond_the_bucketed_range(ctx):
    """64 keys past BKT_KEYS << BKT_MAX_LOG2: the smallest call at 64 bands that takes the HBM table directly again."""
    t0 = time.perf_counter()
    exp_off, exp_pairs = RS.expected("beyond_buckets")
    t1 = time.perf_counter()
    assert RS.n_keys("beyond_buckets") == exp_off.size * 64 - 64 > RS.BUCKET_LIMIT
    assert 0 < len(exp_pairs) < 4 * (len(exp_off) - 1) and exp_off[-1] > exp_off[-2]
    run_set(ctx, "beyond_buckets")
    print("beyond_buckets: yardstick %.1f s, device and comparison %.1f s" % (t1 - t0, time.perf_counter() - t1))


# ---- (b) route changes on one ctx ------------------------------------------------------------------------------------------------
def test_the_routes_one_after_the_other(ctx):
    for name in ("direct_last", "lds_first", "no_key_flood", "lds_first", "direct_last"):
        run_set(ctx, name)


# ---- (c) the table path of a bucketed size ---------------------------------------------------------------------------------------
def child(out):
    """(run in a child process) lds_first's offsets and pairs to the file `out`"""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    off, pairs = run_set(c, "lds_first")
    c.close()
    np.savez(out, off=off, pairs=pairs)


def test_no_buckets_gives_the_same_pairs(ctx, tmp_path):
    """The resolve reads CIRCKIT_UNIQ_NO_BUCKETS once per process: a fresh child takes the HBM table at 2^19 keys."""
    out = str(tmp_path / "no_buckets.npz")
    env = dict(os.environ, CIRCKIT_UNIQ_NO_BUCKETS="1")
    r = subprocess.run([sys.executable, "-c", "import sys; from tests import test_cluster_resolve_gpu as T; T.child(sys.argv[1])", out],
                       cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    got = np.load(out)
    off, pairs = run_set(ctx, "lds_first")                                        # (a)'s: the bucketed route of this process
    assert np.array_equal(got["off"], off) and np.array_equal(got["pairs"], pairs)


# ---- (d) the chain at a bucketed size --------------------------------------------------------------------------------------------
CHAIN = dict(k=21, log2_bins=8)


@functools.lru_cache(maxsize=None)
def short_records():
    """8192 records of 40 .. 60 symbols, 300 of them copies of an earlier one, rotated or reverse-complemented."""
    rng = np.random.default_rng(4201)
    recs = [SS.random_acgt(rng, rng.integers(40, 61)) for _ in range(8192)]
    for i in rng.choice(np.arange(1, 8192), size=300, replace=False):
        recs[int(i)] = S.mutated(rng, recs[int(rng.integers(0, i))], sub=0.0)
    return tuple(recs)


@functools.lru_cache(maxsize=None)
def short_expected():
    from circkit_amd import api
    p = api.cluster_params()
    records = short_records()
    rows, _ = SS.expected(records, CHAIN["k"], CHAIN["log2_bins"])
    keys = N.band_keys(rows, p.n_bands, p.band_bins)
    _, pairs = N.candidates(rows, p.n_bands, p.band_bins, keys=keys)
    match, filled, bad = R.compare_pairs(rows, rows, pairs)
    assert bad == 0
    labels, n_clusters, n_linked, n_invalid = C.link(len(records), [tuple(q) for q in pairs.tolist()], np.stack([match, filled], axis=1).tolist(),
                                                     (p.min_similarity_q16, p.min_filled))
    assert n_invalid == 0
    return keys, np.array(labels, dtype=np.uint64), n_clusters, n_linked


def test_the_chain_on_short_records():
    import circkit_amd
    from circkit_amd import api
    records = short_records()
    keys, exp_labels, n_clusters, n_linked = short_expected()
    assert keys.size == len(records) * api.cluster_params().n_bands >= RS.BUCKET_MIN
    no_key = float((keys == N.NO_KEY).mean())
    print("short records: %.1f %% of the keys are NO_KEY, %d pairs link, %d clusters" % (100 * no_key, n_linked, n_clusters))
    assert no_key >= 0.9 and n_linked >= 100
    labels, m = circkit_amd.cluster_batch(records, **CHAIN)
    assert np.array_equal(labels, exp_labels) and m == n_clusters


# ---- (e) the uniq table belongs to whoever used it last --------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(torch.device("cuda", 0))


def _uniq_status(ctx):
    n = ctypes.c_uint32(0xDEAD)
    rc = ctx._lib.circkit_uniq_status(ctx._h, ctypes.byref(n))
    return rc, n.value


def _stream_keys(seed, n=3000):
    """n records over n // 2 distinct keys and ~0, and their global indices"""
    rng = np.random.default_rng(seed)
    pool = np.append(K.random_keys(rng, n // 2), K.EMPTY)
    h = pool[rng.integers(0, len(pool), size=n)]
    return h, np.arange(n, dtype=np.uint64) + np.uint64(BASE)


def _insert_and_lookup(ctx, h, idx):
    import torch
    n = len(h)
    d_h = _dev(h)
    out = torch.full((n,), LOOKUP_CANARY, dtype=torch.int64, device=torch.device("cuda", 0))
    ctx.uniq_reset(n)
    ctx.uniq_insert_device(d_h, n, int(idx[0]))
    ctx.uniq_lookup_device(d_h, n, out)
    assert _uniq_status(ctx) == (OK, 0)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), K.expected_first_seen(h, idx))


def _overflow(ctx):
    """A table sized for 1 key (1024 slots) and 5000 distinct keys, none ~0: the records beyond the slots found none."""
    h = K.random_keys(np.random.default_rng(4302), 5000)
    ctx.uniq_reset(1)
    ctx.uniq_insert_device(_dev(h), len(h), BASE)
    return len(h) - 1024


def test_candidates_after_a_streaming_uniq(ctx):
    """e1: the table is the stream's, then the candidates', then refused until the next circkit_uniq_reset, then the stream's."""
    import torch
    from circkit_amd import api
    h, idx = _stream_keys(4301)
    _insert_and_lookup(ctx, h, idx)
    G.check_candidates(ctx, "several_earlier")
    d_h = _dev(h)
    out = torch.full((len(h),), LOOKUP_CANARY, dtype=torch.int64, device=torch.device("cuda", 0))
    lib = ctx._lib
    assert lib.circkit_uniq_insert_device(ctx._h, api._ptr(d_h), len(h), BASE) == INVALID_ARG
    assert b"circkit_uniq_reset" in lib.circkit_last_error(ctx._h)
    assert lib.circkit_uniq_lookup_device(ctx._h, api._ptr(d_h), len(h), api._ptr(out)) == INVALID_ARG
    ctx.synchronize()
    assert (out.cpu().numpy().view(np.uint64) == LOOKUP_CANARY).all(), "a refused lookup wrote its output"
    _insert_and_lookup(ctx, h, idx)


def test_candidates_after_a_uniq_overflow(ctx):
    """e2: the resolve clears the count of the overflow before it."""
    lost = _overflow(ctx)
    assert _uniq_status(ctx) == (OOM, lost)
    G.check_candidates(ctx, "several_earlier")
    assert _uniq_status(ctx) == (OK, 0)


def test_a_uniq_overflow_between_the_candidates_and_their_status(ctx):
    """e3: circkit_uniq_status reports the other call's overflow; the candidates' status answers for its own resolve."""
    rows, nb, bb = S.candidate_cases()["several_earlier"]
    exp_off, exp_pairs = S.expected_candidates("several_earlier")
    c = G.Candidates(rows, len(rows) * nb)
    c.launch(ctx, nb, bb)
    lost = _overflow(ctx)
    assert _uniq_status(ctx) == (OOM, lost)
    assert G.candidates_status(ctx) == (OK, len(exp_pairs))
    assert G.candidates_status(ctx) == (OK, len(exp_pairs))
    assert _uniq_status(ctx) == (OOM, lost)
    off, pairs = c.result()
    assert np.array_equal(off, exp_off)
    assert np.array_equal(pairs, S.pair_buffer(exp_off, exp_pairs, c.capacity, G.PAIR_CANARY))


def test_uniq_first_seen_after_the_candidates(ctx):
    """e4: the host streaming form resets the table a resolve left behind by itself; two batches, the second grows the table."""
    G.check_candidates(ctx, "several_earlier")
    h, idx = _stream_keys(4304, 6000)
    exp = K.expected_first_seen(h, idx)
    assert np.array_equal(ctx.uniq_first_seen(h[:3000], BASE), K.expected_first_seen(h[:3000], idx[:3000]))
    assert np.array_equal(ctx.uniq_first_seen(h[3000:], BASE + 3000), exp[3000:])
    assert (exp[3000:] < BASE + 3000).any() and _uniq_status(ctx) == (OK, 0)
