"""GPU: what the host-buffer entry points share -- the order and the text of what they refuse from the offsets alone, staging
buffers that grow and are used again, and the life of a ctx that owns them.  The entry points: circkit_windows_gather,
_windows_translate, _sketch_batch, _sketch_compare, _cluster_batch, _prealign_batch, _distance_pairs, _orfs_batch,
_monomerize_batch, _monomers_batch, _uniq_batch, _fasta_write_text and (staging and lifecycle only) _canonicalize_batch.  Every result is held against the unit's own yardstick
(tests/*_ref.py, oracle); the expected messages are literals."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests import cluster_ref as CR
from tests import distance_ref as DR
from tests import fasta_write_sets as FW
from tests import mono_ref
from tests import monomers_ref as MR
from tests import orfs_ref
from tests import prealign_ref as PR
from tests import seqsets
from tests import sketch_ref as SR
from tests import translate_ref as TR
from tests import uniq_compact_ref as UR
from tests import windows_ref as WR

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, TOO_LONG = 0, -1, -4
K, LOG2_BINS = 4, 4                      # the smallest sketch: records of 5 symbols have k-mers
CLUSTER = dict(n_bands=4, band_bins=2, min_similarity=0.5, min_filled=1)
MONO = dict(seed_len=5, max_mismatch=1)
MAX_DISTANCE = 8
AA = TR.genetic_codes()[1]


@pytest.fixture(scope="module")
def ctx():
    import circkit_amd
    c = circkit_amd.Context(0)
    yield c
    c.close()


# ---- 1. the error contract ---------------------------------------------------------------------------------------------------
L31, L32 = 2 ** 31, 2 ** 32
FIRST = [1, 4, 6, 8]                     # offsets[0] = 1
FALLS = [0, 4, 2, 6]
BOTH = [1, 4, 2, 6]                      # offsets[0] = 1 and a decrease
MSG_FIRST = "offsets[0] must be 0"
MSG_FALLS = "offsets must not decrease"


class Calls:
    """One call of every entry point on a batch of 3 records with room for its outputs; what a case overrides is a keyword.
    The payload is 8 bytes, or the 1 byte of the cases with a record at the limit: no call of this test may get as far as
    reading it."""

    def __init__(self, ctx):
        from circkit_amd import api
        self.api, self.lib, self.h = api, ctx._lib, ctx._h
        self.data8, self.data1 = np.zeros(8, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        self.win = WR.windows([(2, 0, 0, 0)])
        self.pairs = np.array([[0, 1]], dtype=np.uint32)
        self.out8, self.u64x4, self.u64x3, self.u32x4 = (np.zeros(8, dtype=np.uint8), np.zeros(4, dtype=np.uint64), np.zeros(3, dtype=np.uint64),
                                                         np.zeros(4, dtype=np.uint32))
        self.rows, self.fs = np.zeros(3 << LOG2_BINS, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        self.window_out = np.zeros(1, dtype=WR.WINDOW_DTYPE)
        self.orfs = np.zeros(4, dtype=api.ORF_DTYPE)
        self.head = np.array([[0, 1], [1, 1], [2, 1]], dtype=np.uint64)
        self.total = ctypes.c_uint64(0)
        self.kept = []

    def error(self):
        return self.lib.circkit_last_error(self.h).decode()

    def _p(self, x):
        return None if x is None else x.ctypes.data if isinstance(x, np.ndarray) else ctypes.byref(x)

    def _offs(self, v):
        """the address of v as a uint64 array, which lives as long as this object (two of them never share an address)"""
        self.kept.append(np.array(v, dtype=np.uint64))
        return self.kept[-1].ctypes.data

    def windows_gather(self, offs, data=None, out_off="given"):
        out_off = self.u64x4 if isinstance(out_off, str) else out_off
        return self.lib.circkit_windows_gather(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, self._p(self.win), 1,
                                               self._p(self.out8), 8, self._p(out_off), ctypes.byref(self.total))

    def windows_translate(self, offs, first_as_m=0):
        p = self.api.translate_params(table=AA)
        p.first_as_m = first_as_m
        return self.lib.circkit_windows_translate(self.h, self._p(self.data8), self._offs(offs), 3, self._p(self.win), 1, ctypes.byref(p),
                                                  self._p(self.out8), 8, self._p(self.u64x4), ctypes.byref(self.total))

    def sketch_batch(self, offs, data=None, k=K):
        p = self.api.sketch_params(k=k, log2_bins=LOG2_BINS)
        return self.lib.circkit_sketch_batch(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, ctypes.byref(p),
                                             self._p(self.rows), self._p(self.u32x4))

    def cluster_batch(self, offs, data=None, n_bands=4):
        sp, p = self.api.sketch_params(k=K, log2_bins=LOG2_BINS), self.api.cluster_params(**dict(CLUSTER, n_bands=n_bands))
        return self.lib.circkit_cluster_batch(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, ctypes.byref(sp),
                                              ctypes.byref(p), self._p(self.u64x3), ctypes.byref(self.total))

    def prealign_batch(self, offs, data=None, min_votes=1):
        sp = self.api.sketch_params(k=K, log2_bins=LOG2_BINS)
        return self.lib.circkit_prealign_batch(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, ctypes.byref(sp),
                                               self._p(self.pairs), 1, min_votes, self._p(self.window_out), self._p(self.u32x4))

    def distance_pairs(self, offs_a, offs_b, data=None, max_distance=MAX_DISTANCE):
        p = self.api.distance_params(max_distance=max_distance)
        data = self.data8 if data is None else data
        return self.lib.circkit_distance_pairs(self.h, self._p(data), self._offs(offs_a), 3, self._p(data), self._offs(offs_b), 3,
                                               ctypes.byref(p), self._p(self.pairs), 1, self._p(self.u32x4), self._p(self.u64x3.view(np.uint32)))

    def orfs_batch(self, offs, params="given"):
        p = self.api.orf_params() if isinstance(params, str) else params
        return self.lib.circkit_orfs_batch(self.h, self._p(self.data8), self._offs(offs), 3, self._p(p), self._p(self.u64x4), self._p(self.orfs), 4,
                                           ctypes.byref(self.total))

    def monomerize_batch(self, offs, data=None, seed_len=5):
        p = self.api.monomerize_params(**dict(MONO, seed_len=seed_len))
        return self.lib.circkit_monomerize_batch(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, ctypes.byref(p),
                                                 self._p(self.u32x4))

    def monomers_batch(self, offs, data=None, seed_len=5):
        p, f = self.api.monomerize_params(**dict(MONO, seed_len=seed_len)), self.api.monomer_filter()
        return self.lib.circkit_monomers_batch(self.h, self._p(self.data8 if data is None else data), self._offs(offs), 3, ctypes.byref(p),
                                               ctypes.byref(f), None, self._p(self.out8), self._p(self.u64x4), self._p(self.u64x3), self._p(self.u32x4),
                                               ctypes.byref(self.total))

    def uniq_batch(self, offs, out_off="given"):
        out_off = self.u64x4 if isinstance(out_off, str) else out_off
        return self.lib.circkit_uniq_batch(self.h, self._p(self.data8), self._offs(offs), 3, 0, self._p(self.out8), self._p(out_off),
                                           self._p(self.u64x3), self._p(self.fs), ctypes.byref(self.total))

    def fasta_write_text(self, body_offs, out_off="given"):
        out_off = self.u64x4 if isinstance(out_off, str) else out_off
        return self.lib.circkit_fasta_write_text(self.h, self._p(self.data8), 8, self._p(self.head), None, 3, None, 3, None, self._p(self.data8),
                                                 self._offs(body_offs), 3, self._p(self.out8), 8, self._p(out_off), ctypes.byref(self.total))


def at_limit(limit, record=1):
    """3 records, `record` of exactly `limit` symbols, the others of 1 and 0: the offsets of a 1-byte payload but for that one"""
    lengths = [1, 0, 0]
    lengths[record] = limit
    return [0] + np.cumsum(lengths).tolist()


def too_long(what, record=1):
    return "record %d has 2^31 symbols or more: %s" % (record, what)


MSG_2_32 = "a record of 2^32 symbols or more"
ONE = "data1"                            # the case runs on the 1-byte payload


def cases():
    """(entry point, arguments, keywords, return code, message)"""
    out = []
    for name in ("windows_gather", "windows_translate", "sketch_batch", "cluster_batch", "prealign_batch", "monomerize_batch", "monomers_batch",
                 "uniq_batch"):
        out += [(name, (FIRST,), {}, INVALID_ARG, MSG_FIRST), (name, (FALLS,), {}, INVALID_ARG, MSG_FALLS),
                (name, (BOTH,), {}, INVALID_ARG, MSG_FIRST)]                      # two faults: offsets[0] is looked at before the walk
    good = [0, 2, 4, 6]
    for name, what in (("sketch_batch", "nothing was sketched"), ("cluster_batch", "nothing was clustered"), ("prealign_batch", "nothing was aligned")):
        out += [(name, (at_limit(L31),), {"data": ONE}, TOO_LONG, too_long(what)),
                (name, (at_limit(L31 - 1, 0)[:2] + [L31 - 1 + L31, 2 * L31],), {"data": ONE}, TOO_LONG, too_long(what)),     # one below, then at
                (name, ([0, 4, 2, 2 + L31],), {}, INVALID_ARG, MSG_FALLS),        # two faults: the lower record
                (name, ([0, L31, 5, 6],), {"data": ONE}, TOO_LONG, too_long(what, 0)),
                (name, ([0, L32 + 7, 3, 9],), {"data": ONE}, TOO_LONG, too_long(what, 0)),
                (name, ([0, 1, 0, L32],), {"data": ONE}, INVALID_ARG, MSG_FALLS)]
    out += [("sketch_batch", (BOTH,), {"k": 3}, INVALID_ARG, "k must be 4 .. 32"),                  # the params before the offsets
            ("cluster_batch", (BOTH,), {"n_bands": 0}, INVALID_ARG, "n_bands must be 1 .. 64"),
            ("prealign_batch", (BOTH,), {"min_votes": 0}, INVALID_ARG, "min_votes must be at least 1"),
            ("windows_translate", (BOTH,), {"first_as_m": 2}, INVALID_ARG, "first_as_m must be 0 or 1"),
            ("windows_gather", (BOTH,), {"out_off": None}, INVALID_ARG, "null buffer"),              # the null buffers before the offsets
            ("uniq_batch", (BOTH,), {"out_off": None}, INVALID_ARG, "null buffer")]
    what = "no distance was computed"
    out += [("distance_pairs", (FIRST, good), {}, INVALID_ARG, MSG_FIRST), ("distance_pairs", (good, FIRST), {}, INVALID_ARG, MSG_FIRST),
            ("distance_pairs", (FALLS, good), {}, INVALID_ARG, MSG_FALLS), ("distance_pairs", (good, FALLS), {}, INVALID_ARG, MSG_FALLS),
            ("distance_pairs", (at_limit(L31), [0, 1, 1, 1]), {"data": ONE}, TOO_LONG, too_long(what)),
            ("distance_pairs", ([0, 1, 1, 1], at_limit(L31, 2)), {"data": ONE}, TOO_LONG, too_long(what, 2)),
            ("distance_pairs", (FALLS, FIRST), {}, INVALID_ARG, MSG_FALLS),       # two faults: batch a before batch b
            ("distance_pairs", (FIRST, FALLS), {}, INVALID_ARG, MSG_FIRST),
            ("distance_pairs", (BOTH, BOTH), {"max_distance": 256}, INVALID_ARG, "max_distance must be 0 .. 255")]
    for name in ("monomerize_batch", "monomers_batch"):
        out += [(name, (at_limit(L32),), {"data": ONE}, TOO_LONG, MSG_2_32),
                (name, ([0, L32 - 1, L32 - 1, L32 - 1 + L32],), {"data": ONE}, TOO_LONG, MSG_2_32),
                (name, ([0, 4, 2, 2 + L32],), {}, INVALID_ARG, MSG_FALLS),
                (name, (BOTH,), {"seed_len": 0}, INVALID_ARG, MSG_FIRST),         # offsets[0], then the params, then the walk
                (name, (FALLS,), {"seed_len": 0}, INVALID_ARG, "Seed length must be at least 1 and at most 63")]
    out += [("orfs_batch", (FIRST,), {}, INVALID_ARG, MSG_FIRST), ("orfs_batch", (BOTH,), {"params": None}, INVALID_ARG, MSG_FIRST),
            ("fasta_write_text", (FALLS,), {}, INVALID_ARG, "body_offsets must not decrease"),
            ("fasta_write_text", (FALLS,), {"out_off": None}, INVALID_ARG, "null buffer")]
    return out


def test_the_error_contract(ctx):
    """Return code and circkit_last_error of every host-buffer entry point on 3 records whose offsets are wrong: offsets[0] = 1,
    offsets that fall, a record of exactly the unit's limit, and two faults at once.  Every case returns before the entry point
    reads a payload byte or enqueues anything (read off the source), so no kernel sees these offsets.  Left out for that reason:
      * a record at a limit for circkit_windows_gather, _windows_translate, _uniq_batch and _orfs_batch: they have no limit of
        their own, the call would copy 2^31 bytes out of the 1-byte payload;
      * falling offsets for circkit_orfs_batch: it does not walk the offsets, the batch would reach the count kernel;
      * offsets[0] = 1 for circkit_fasta_write_text: a body may begin behind bytes of no record, that is no fault; and a record
        at a limit, of which it has none;
      * circkit_sketch_compare, which takes no offsets.
    (A length of 2^31 - 1, of 2^32 - 1 and "no limit" are accepted: those are tests/test_csr_walk_cpu.py's, here they would
    need the payload.)"""
    calls = Calls(ctx)
    seen = set()
    for name, args, kw, code, message in cases():
        kw = {k: (calls.data1 if v is ONE else v) for k, v in kw.items()}
        rc = getattr(calls, name)(*args, **kw)
        assert (rc, calls.error()) == (code, message), (name, args, sorted(kw))
        seen.add(name)
    assert len(seen) == 11
    ctx.synchronize()
    # and the ctx is as good as new: the same entry points take a batch
    recs = batch("small")
    for unit in UNITS:
        assert_same(unit(ctx, recs), expected(unit.__name__, "small"), unit.__name__)


# ---- 2. grow and reuse ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(name):
    """small: 3 records of 5 .. 40 symbols; large: 150 of them.  Every third record is a rotation or the reverse complement of an
    earlier one, every fifth a unit written twice and a bit (a multimer)."""
    rng = np.random.default_rng({"small": 5, "large": 6}[name])
    recs = []
    for i in range({"small": 3, "large": 150}[name]):
        n = int(rng.integers(5, 41))
        if i % 3 == 2:
            src = recs[int(rng.integers(0, i))]
            k = int(rng.integers(0, len(src)))
            r = src[k:] + src[:k] if rng.random() < 0.5 else O.revcomp(src)
        elif i % 5 == 4:
            unit = FW.letters(rng, max(n // 3, 5))
            r = (unit * 3)[:max(n, 2 * len(unit) + 2)][:40]
        else:
            r = FW.letters(rng, n)
        recs.append(r)
    assert all(5 <= len(r) <= 40 for r in recs)
    return tuple(recs)


def pack(recs):
    data = np.frombuffer(b"".join(recs), dtype=np.uint8)
    return data, np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.uint64)


def some_pairs(n, m):
    """m pairs of records below n, every record named, some pairs twice"""
    return [(p % n, (7 * p + 1) % n) for p in range(m)]


def some_windows(recs):
    """two windows a record, one a strand, longer than the record now and then (they wrap); a multiple of 3 for the translate"""
    rows = []
    for i, r in enumerate(recs):
        rows += [(3 * ((len(r) + 2 * i) % 17 + 1), i, (5 * i) % len(r), 0), (3 * (i % 9), i, i % len(r), 1)]
    return WR.windows(rows)


def other(recs):
    """a second batch for the entry points that take two: the records the other way round, each rotated by one"""
    return tuple(r[1:] + r[:1] for r in reversed(recs))


def fasta_case(recs, raw):
    """the records as a FASTA text with their heads; written either from the raw spans, or from the batch as the body, the heads
    through a map the other way round, every output with a label"""
    heads = [b"rec%d of %d" % (i, len(r)) for i, r in enumerate(recs)]
    text, hs, rs = FW.layout(heads, list(recs))
    if raw:
        return FW.Case("raw", text, hs, raw=rs)
    n = len(recs)
    data, offs = pack(recs)
    return FW.Case("body", text, hs, body=data.tobytes(), offsets=offs, src=np.arange(n - 1, -1, -1), labels=FW.windows([(i, 3 * i, i & 1) for i in range(n)]))


def windows_gather(ctx, recs):
    return ctx.windows_gather(*pack(recs), some_windows(recs))


def windows_translate(ctx, recs):
    return ctx.windows_translate(*pack(recs), some_windows(recs), table=AA, unknown="X", first_as_m=True)


def sketch_batch(ctx, recs):
    return ctx.sketch_batch(*pack(recs), k=K, log2_bins=LOG2_BINS)


def sketch_compare(ctx, recs):
    n = len(recs)
    return ctx.sketch_compare(SR.sketch_batch(recs, K, LOG2_BINS)[0], SR.sketch_batch(other(recs), K, LOG2_BINS)[0], some_pairs(n, 2 * n))


def cluster_batch(ctx, recs):
    return ctx.cluster_batch(*pack(recs), k=K, log2_bins=LOG2_BINS, **CLUSTER)


def prealign_batch(ctx, recs):
    return ctx.prealign_batch(*pack(recs), some_pairs(len(recs), 2 * len(recs)), k=K, log2_bins=LOG2_BINS, min_votes=1)


def distance_pairs(ctx, recs):
    return ctx.distance_pairs(*pack(recs), *pack(other(recs)), some_pairs(len(recs), 2 * len(recs)), max_distance=MAX_DISTANCE)


def orfs_batch(ctx, recs):
    got = ctx.orfs_batch(*pack(recs), strands=3, mode=0)
    return tuple(got[f] for f in ("offsets", "start", "stop", "length", "wraps", "strand"))


def monomerize_batch(ctx, recs):
    return (ctx.monomerize_batch(*pack(recs), **MONO),)


def monomers_batch(ctx, recs):
    full = np.array([len(r) + i % 3 for i, r in enumerate(recs)], dtype=np.uint64)
    return ctx.monomers_batch(*pack(recs), full_len=full, **MONO)


def uniq_batch(ctx, recs):
    return ctx.uniq_batch(*pack(recs), canonicalize=False) + ctx.uniq_batch(*pack(recs), canonicalize=True)


def fasta_write_text(ctx, recs):
    out = ()
    for raw in (False, True):
        c = fasta_case(recs, raw)
        text, off = ctx.fasta_write_text(c.text, c.head, body=c.body, offsets=c.offsets, raw=c.raw, src=c.src, labels=c.labels)
        out += (np.frombuffer(text, dtype=np.uint8), off)
    return out


def canonicalize_batch(ctx, recs):
    got = ctx.canonicalize_batch(*pack(recs), want_bytes=True, want_index=True, want_strand=True, want_xxh3=True)
    return tuple(got[f] for f in ("bytes", "index", "strand", "xxh3"))


UNITS = (windows_gather, windows_translate, sketch_batch, sketch_compare, cluster_batch, prealign_batch, distance_pairs, orfs_batch, monomerize_batch,
         monomers_batch, uniq_batch, fasta_write_text, canonicalize_batch)


@functools.lru_cache(maxsize=None)
def expected(unit, name):
    """the yardstick's answer in the shape the function of that name above returns; computed once and left unchanged"""
    recs = batch(name)
    data, offs = pack(recs)
    n = len(recs)
    if unit == "windows_gather":
        out, off, bad = WR.gather(data, offs, some_windows(recs))
        assert bad == 0
        return out, off
    if unit == "windows_translate":
        out, off, bad = TR.windows_translate(data, offs, some_windows(recs), AA, b"X", True)
        assert bad == 0
        return out, off
    if unit == "sketch_batch":
        return SR.sketch_batch(recs, K, LOG2_BINS)
    if unit == "sketch_compare":
        return SR.compare_pairs(SR.sketch_batch(recs, K, LOG2_BINS)[0], SR.sketch_batch(other(recs), K, LOG2_BINS)[0], some_pairs(n, 2 * n))[:2]
    if unit == "cluster_batch":
        rows = SR.sketch_batch(recs, K, LOG2_BINS)[0]
        _, pairs = CR.candidates(rows, CLUSTER["n_bands"], CLUSTER["band_bins"])
        match, filled, _ = SR.compare_pairs(rows, rows, pairs)
        labels, m, _, bad = CR.link(n, pairs, list(zip(match, filled)), (CR.q16(CLUSTER["min_similarity"]), CLUSTER["min_filled"]))
        assert bad == 0
        return np.array(labels, dtype=np.uint64), m
    if unit == "prealign_batch":
        rows, _, anc = PR.anchors_batch(recs, K, LOG2_BINS)
        w, sc, _, bad = PR.pairs(rows, anc, [len(r) for r in recs], K, 1, some_pairs(n, 2 * n))
        assert bad == 0
        return w, sc
    if unit == "distance_pairs":
        d, sc, _, bad = DR.pairs(list(recs), list(other(recs)), some_pairs(n, 2 * n), MAX_DISTANCE)
        assert bad == 0
        return d, sc
    if unit == "orfs_batch":
        eo, e = orfs_ref.orfs_batch(data, offs, threads=16)
        return (eo,) + tuple(e[f] for f in ("start", "stop", "length", "wraps", "strand"))
    if unit == "monomerize_batch":
        return (mono_ref.batch(data, offs, threads=16, **MONO),)
    if unit == "monomers_batch":
        full = np.array([len(r) + i % 3 for i, r in enumerate(recs)], dtype=np.uint64)
        return MR.compact(data, offs, mono_ref.batch(data, offs, threads=16, **MONO), full)
    if unit == "uniq_batch":
        canon, hashes = O.canonicalize_batch(data, offs, True, True, threads=16)
        fs = O.uniq_first_seen(hashes)
        return tuple(UR.compact(data, offs, fs)[:3]) + (fs,) + tuple(UR.compact(canon, offs, fs)[:3]) + (fs,)
    if unit == "fasta_write_text":
        out = ()
        for raw in (False, True):
            recs_out, bad = FW.expected(fasta_case(recs, raw))
            assert bad == 0
            out += (np.frombuffer(b"".join(recs_out), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(r) for r in recs_out])]).astype(np.uint64))
        return out
    if unit == "canonicalize_batch":
        canon, hashes = O.canonicalize_batch(data, offs, True, True, threads=16)
        per_record = [seqsets.expected(O, r) for r in recs]
        return canon, np.array([idx for _, _, idx in per_record], dtype=np.uint32), np.array([st for _, st, _ in per_record], dtype=np.uint8), hashes
    raise KeyError(unit)


def assert_same(got, exp, what):
    assert len(got) == len(exp), what
    for k, (g, e) in enumerate(zip(got, exp)):
        if isinstance(e, np.ndarray):
            assert g.dtype == e.dtype or g.dtype.itemsize == e.dtype.itemsize, (what, k, g.dtype, e.dtype)
            assert g.shape == e.shape and np.array_equal(g, e), (what, k)
        else:
            assert g == e, (what, k)


@pytest.mark.parametrize("unit", UNITS, ids=lambda u: u.__name__)
def test_grow_and_reuse(ctx, unit):
    """One ctx: a small batch, one 50 times larger (every staging buffer of the entry point is regrown), the small one again
    (in buffers that are now larger than it needs)."""
    for name in ("small", "large", "small"):
        assert_same(unit(ctx, batch(name)), expected(unit.__name__, name), (unit.__name__, name))


def test_each_windows_status_answers_for_its_own_kind(ctx):
    """A gather, then a translate on the same ctx: circkit_windows_status still reports the gather, circkit_translate_status the
    translate, whatever the order in which they are asked."""
    recs = batch("large")
    g, t = expected("windows_gather", "large"), expected("windows_translate", "large")
    assert len(g[0]) != len(t[0])
    assert_same(windows_gather(ctx, recs), g, "gather")
    assert_same(windows_translate(ctx, recs), t, "translate")
    assert ctx.windows_status() == (len(g[0]), 0)
    assert ctx.translate_status() == (len(t[0]), 0)
    assert ctx.windows_status() == (len(g[0]), 0)
    assert_same(windows_gather(ctx, batch("small")), expected("windows_gather", "small"), "gather, small")
    assert ctx.translate_status() == (len(t[0]), 0)
    assert ctx.windows_status() == (len(expected("windows_gather", "small")[0]), 0)


# ---- 3. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_a_ctx_that_touched_no_unit():
    import circkit_amd
    for _ in range(3):
        c = circkit_amd.Context(0)
        c.close()
        c.close()                                              # (closed is closed)


def test_a_ctx_that_ran_every_host_form():
    import circkit_amd
    c = circkit_amd.Context(0)
    try:
        recs = batch("small")
        for unit in UNITS:
            assert_same(unit(c, recs), expected(unit.__name__, "small"), unit.__name__)
    finally:
        c.close()


def test_two_ctxs_alternately():
    """Two ctxs at a time, each with unit state of its own; one is destroyed and made again three times over, the other goes on
    working between and after."""
    import circkit_amd
    small, large = batch("small"), batch("large")
    survivor = circkit_amd.Context(0)
    try:
        for turn in range(3):
            other_ctx = circkit_amd.Context(0)
            try:
                for unit in (sketch_batch, distance_pairs, uniq_batch, windows_gather):
                    assert_same(unit(other_ctx, large if turn == 1 else small), expected(unit.__name__, "large" if turn == 1 else "small"), unit.__name__)
                    assert_same(unit(survivor, small), expected(unit.__name__, "small"), unit.__name__)
            finally:
                other_ctx.close()
            assert_same(cluster_batch(survivor, large), expected("cluster_batch", "large"), "survivor")
        for unit in UNITS:
            assert_same(unit(survivor, small), expected(unit.__name__, "small"), unit.__name__)
    finally:
        survivor.close()
