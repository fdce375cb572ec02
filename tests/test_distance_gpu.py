"""GPU: circkit_distance_pairs_device / _status, circkit_distance_pairs and the drivers' flags that use them
(circkit_amd/cluster.py --min-identity / --max-distance, circkit_amd/prealign.py --max-distance) against the yardstick
tests/distance_ref.py, exactly: every distance, score and total.  The input sets are tests/distance_sets.py's, the ones the CPU
fiber test runs, and the ones that are too large for the fibers; canaries surround every output and follow every payload."""
import ctypes

import numpy as np
import pytest

from tests import distance_ref as D
from tests import distance_sets as S

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY32, CANARY8, TAIL = 0x3F3F3F3F, 0x3F, 0x4E
OK, INVALID_ARG, TOO_LONG = 0, -1, -4
OVER = D.OVER


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(_dev())                  # (a copy: the sets' arrays are read-only views)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)


@pytest.fixture(scope="module")
def ctx():
    """A ctx that launches on torch's current stream, so that the tensors torch fills and the ctx's kernels are ordered."""
    import circkit_amd
    import torch
    c = circkit_amd.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def distance_status(ctx):
    a, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_distance_status(ctx._h, ctypes.byref(a), ctypes.byref(bad))
    return rc, a.value, bad.value


class Pairs:
    """A Case on the device: GUARD canary bytes behind either payload, canaries round the distances and the scores (0x3F)."""

    def __init__(self, case):
        import torch
        self.case = case
        self.pairs = np.ascontiguousarray(np.asarray(case.pairs, dtype=np.uint64).astype(np.uint32)).reshape(-1, 2)
        self.m = len(self.pairs)
        self.n_a, self.n_b = len(case.off_a) - 1, len(case.off_b) - 1
        self.data_a = np.concatenate([case.data_a, np.full(GUARD, TAIL, dtype=np.uint8)])
        self.d_data_a, self.d_off_a = _to(self.data_a), _to(_i64(case.off_a))
        if case.same:
            self.data_b, self.d_data_b, self.d_off_b = self.data_a, self.d_data_a, self.d_off_a
        else:
            self.data_b = np.concatenate([case.data_b, np.full(GUARD, TAIL, dtype=np.uint8)])
            self.d_data_b, self.d_off_b = _to(self.data_b), _to(_i64(case.off_b))
        self.d_pairs = _to(_i32(self.pairs).reshape(-1)) if self.m else None
        self.d_dist = torch.full((GUARD + self.m + GUARD,), CANARY32, dtype=torch.int32, device=_dev())
        self.d_scores = torch.full((2 * GUARD + 2 * self.m + 2 * GUARD,), CANARY32, dtype=torch.int32, device=_dev())

    def launch(self, ctx, W=None):
        out = self.case.out
        ctx.distance_pairs_device(self.d_data_a, self.d_off_a, self.n_a, self.d_data_b, self.d_off_b, self.n_b, self.d_pairs, self.m,
                                  self.d_dist[GUARD:] if out != "scores" else None, self.d_scores[2 * GUARD:] if out != "distance" else None,
                                  max_distance=self.case.W if W is None else W)

    def result(self):
        """(distance, scores) after the canary checks; an output that was not asked for is untouched."""
        dist, sc = self.d_dist.cpu().numpy().view(np.uint32), self.d_scores.cpu().numpy().view(np.uint32)
        assert (dist[:GUARD] == CANARY32).all() and (dist[GUARD + self.m:] == CANARY32).all(), "distances written outside the n_pairs"
        assert (sc[:2 * GUARD] == CANARY32).all() and (sc[2 * GUARD + 2 * self.m:] == CANARY32).all(), "scores written outside the n_pairs"
        assert np.array_equal(self.d_data_a.cpu().numpy(), self.data_a) and np.array_equal(self.d_data_b.cpu().numpy(), self.data_b), "a payload changed"
        assert np.array_equal(self.d_off_a.cpu().numpy().view(np.uint64), self.case.off_a) and np.array_equal(self.d_off_b.cpu().numpy().view(np.uint64), self.case.off_b)
        if self.m:
            assert np.array_equal(self.d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), self.pairs)
        dist, sc = dist[GUARD:GUARD + self.m].copy(), sc[2 * GUARD:2 * GUARD + 2 * self.m].reshape(-1, 2).copy()
        if self.case.out == "scores":
            assert (dist == CANARY32).all()
        if self.case.out == "distance":
            assert (sc == CANARY32).all()
        return dist, sc


def _case(name):
    return S.past_the_grid() if name == "past_the_grid" else S.planted()[0] if name == "planted" else S.cases()[name]


def check(ctx, name):
    """The set on the card, twice: every distance, score and total, and the same bits the second time."""
    case = _case(name)
    dist, scores, within, invalid = S.expected(name)
    v = Pairs(case)
    v.launch(ctx)
    rc, got_within, got_invalid = distance_status(ctx)
    got_d, got_s = v.result()
    assert (rc, got_within, got_invalid) == (INVALID_ARG if invalid else OK, within, invalid), name
    if case.out != "scores":
        assert np.array_equal(got_d, dist), (name, np.flatnonzero(got_d != dist)[:8])
    if case.out != "distance":
        assert np.array_equal(got_s, scores), name
    v.d_dist[GUARD:GUARD + v.m] = 0x11111111 if case.out != "scores" else CANARY32
    v.d_scores[2 * GUARD:2 * GUARD + 2 * v.m] = 0x11111111 if case.out != "distance" else CANARY32
    v.launch(ctx)
    assert distance_status(ctx) == (rc, got_within, got_invalid), name
    again_d, again_s = v.result()
    assert np.array_equal(again_d, got_d) and np.array_equal(again_s, got_s), name
    return v


@pytest.mark.parametrize("name", sorted(S.cases()) + ["past_the_grid", "planted"])
def test_sets(ctx, name):
    check(ctx, name)


def test_the_status_is_its_own(ctx):
    """A sketch, a compare and a prealign call between a call and its status change nothing of the distance's totals."""
    import torch
    from tests import prealign_sets as PS
    check(ctx, "invalid")
    mine = (INVALID_ARG,) + tuple(S.expected("invalid")[2:])
    assert mine[2] == 5
    rows, anc, lengths, k, mv, pairs = PS.vote_cases()["rotations"]
    n, m = len(rows), len(pairs)
    seqs = [PS.rand_seq(__import__("random").Random(3), 60)] * 4
    data, offs = PS.csr(seqs)
    d_rows4 = torch.empty(4 * 32, dtype=torch.int64, device=_dev())
    ctx.sketch_batch_device(_to(data), _to(_i64(offs)), 4, d_rows4, k=8, log2_bins=5)
    assert ctx.sketch_status()[1] == 0
    assert distance_status(ctx) == mine
    d_rows, d_anc = _to(_i64(rows).reshape(-1)), _to(_i32(anc).reshape(-1))
    d_pairs = _to(_i32(np.asarray(pairs, dtype=np.uint32)).reshape(-1))
    d_sc = torch.empty(2 * m, dtype=torch.int32, device=_dev())
    ctx.sketch_compare_device(d_rows, n, d_rows, n, 5, d_pairs, m, d_sc)
    assert ctx.sketch_compare_status() == 0
    d_win = torch.empty(24 * m, dtype=torch.uint8, device=_dev())
    ctx.prealign_pairs_device(d_rows, d_anc, _to(_i64(PS.offsets_of(lengths))), n, d_pairs, m, d_win, d_sc, k=k, log2_bins=5, min_votes=mv)
    assert ctx.prealign_status()[1] == 0
    assert distance_status(ctx) == mine
    check(ctx, "self_pairs")
    assert distance_status(ctx) == (OK,) + tuple(S.expected("self_pairs")[2:])


def test_argument_errors_change_nothing(ctx):
    import torch
    from circkit_amd import api
    v = check(ctx, "two_batches")
    before = distance_status(ctx)
    dist0, sc0 = v.d_dist.clone(), v.d_scores.clone()
    assert (dist0[:GUARD] == CANARY32).all()
    lib, h = ctx._lib, ctx._h
    DI, SC = v.d_dist[GUARD:], v.d_scores[2 * GUARD:]

    def call(p=None, ba=v.d_data_a, oa=v.d_off_a, na=v.n_a, bb=v.d_data_b, ob=v.d_off_b, nb=v.n_b, pairs=v.d_pairs, m=v.m, di=DI, sc=SC):
        p = p or api.distance_params(max_distance=5)
        return lib.circkit_distance_pairs_device(h, api._ptr(ba), api._ptr(oa), na, api._ptr(bb), api._ptr(ob), nb, ctypes.byref(p), api._ptr(pairs), m,
                                                 api._ptr(di), api._ptr(sc))

    bad = [api.distance_params(max_distance=256), api.distance_params(max_distance=2 ** 32 - 1)]
    for word in range(3):
        r = api.distance_params(max_distance=5)
        r.reserved[word] = 1
        bad.append(r)
    for p in bad:
        assert call(p=p) == INVALID_ARG
    assert lib.circkit_distance_pairs_device(h, api._ptr(v.d_data_a), api._ptr(v.d_off_a), v.n_a, api._ptr(v.d_data_b), api._ptr(v.d_off_b), v.n_b, None,
                                             api._ptr(v.d_pairs), v.m, api._ptr(DI), api._ptr(SC)) == INVALID_ARG
    for kw in (dict(di=None, sc=None), dict(ba=None), dict(oa=None), dict(bb=None), dict(ob=None), dict(pairs=None), dict(na=2 ** 32), dict(nb=2 ** 32)):
        assert call(**kw) == INVALID_ARG, kw
    # an output over the offsets, the pairs or the other output
    for kw in (dict(di=v.d_off_a), dict(sc=v.d_off_a), dict(di=v.d_off_b), dict(sc=v.d_off_b), dict(di=v.d_pairs), dict(sc=v.d_pairs), dict(di=SC), dict(sc=DI)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(di=v.d_data_a[1:]) == INVALID_ARG                                        # the outputs are 4-byte aligned
    assert distance_status(ctx) == before
    assert torch.equal(v.d_dist, dist0) and torch.equal(v.d_scores, sc0)
    v.result()
    assert call(m=0, pairs=None, di=None, sc=None) == OK                                  # no pairs: valid
    assert distance_status(ctx) == (OK, 0, 0)
    # the host form: refused from the offsets alone, before anything is copied
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    di, sc = np.full(1, 7, dtype=np.uint32), np.full(2, 7, dtype=np.uint32)
    good = np.array([0, 5, 10], dtype=np.uint64)
    p = api.distance_params(max_distance=5)

    def host(oa=good, ob=good, p=p, di=di, sc=sc):
        return lib.circkit_distance_pairs(h, api._ptr(data), api._ptr(oa), 2, api._ptr(data), api._ptr(ob), 2, ctypes.byref(p), api._ptr(pairs), 1, api._ptr(di),
                                          api._ptr(sc))

    for offs, code in (([0, 10, 10 + 2 ** 31], TOO_LONG), ([1, 10, 10], INVALID_ARG), ([0, 10, 4], INVALID_ARG)):
        offs = np.array(offs, dtype=np.uint64)
        assert host(oa=offs) == code and host(ob=offs) == code
    assert host(p=bad[0]) == INVALID_ARG and host(di=None, sc=None) == INVALID_ARG
    assert (di == 7).all() and (sc == 7).all()
    assert host() == OK and di[0] == D.lev(b"ACGTA", b"CGTAC") and tuple(sc) == (5 - di[0], 5)


def test_the_host_form(ctx):
    import circkit_amd
    cases = S.cases()
    for name in ("lengths", "repeats", "bytes", "cutoff_32", "two_batches", "self_pairs", "stage_limit"):
        c = cases[name]
        got = circkit_amd.edit_distances(c.a, c.b, c.pairs, max_distance=c.W)
        assert got.dtype == np.uint32 and np.array_equal(got, S.expected(name)[0]), name
        d, sc = circkit_amd.default_context().distance_pairs(c.data_a[c.off_a[0]:], c.off_a - c.off_a[0], *((None, None) if c.same else
                                                             (c.data_b[c.off_b[0]:], c.off_b - c.off_b[0])), c.pairs, max_distance=c.W)
        assert np.array_equal(d, S.expected(name)[0]) and np.array_equal(sc, S.expected(name)[1]), name
    assert circkit_amd.DISTANCE_OVER == OVER and circkit_amd.edit_distances([b"kitten"], [b"sitting"], [(0, 0)]).tolist() == [3]
    assert circkit_amd.edit_distances([b"kitten"], [b"sitting"], [(0, 0)], max_distance=2).tolist() == [OVER]
    assert len(circkit_amd.edit_distances([], None, [])) == 0
    with pytest.raises(circkit_amd.CirckitError):
        circkit_amd.edit_distances([b"ACGT"], None, [(0, 1)])


def test_the_planted_set_end_to_end(ctx):
    """prealign_batch -> windows_gather -> edit_distances: every copy, cut by the window the card finds, is as far from its founder
    as the full table says, and no further than its planted substitutions."""
    import circkit_amd
    from tests import prealign_sets as PS
    records, plants = PS.planted()
    case, counts = S.planted()
    pairs = [(fi, ci) for fi, ci, _, _, _ in plants]
    w, _ = circkit_amd.prealign_batch(records, pairs)
    data, offsets = PS.csr(records)
    out, out_off = circkit_amd.default_context().windows_gather(data, offsets, w)
    out = out.tobytes()
    cut = [out[int(out_off[p]):int(out_off[p + 1])] for p in range(len(pairs))]
    assert cut == case.b                                       # the card's windows are the yardstick's
    got = circkit_amd.edit_distances(records, cut, case.pairs, max_distance=64)
    assert np.array_equal(got, S.expected("planted")[0])
    assert (got <= np.array(counts)).all() and (got > 0).all()


def _text(records):
    return b"".join(b">rec%d planted words\n" % i + r[:70] + b"\n" + r[70:] + b"\n" for i, r in enumerate(records))


@pytest.fixture(scope="module")
def families():
    """The planted families and twelve unrelated records; the yardsticks' sketches, anchors and candidate pairs."""
    import random
    from tests import cluster_ref as C
    from tests import prealign_ref as P
    from tests import prealign_sets as PS
    records, _ = PS.planted()
    rng = random.Random(5)
    records = list(records) + [PS.rand_seq(rng, rng.randint(200, 900)) for _ in range(12)]
    rows, _, anc = P.anchors_batch(records, 21, 8)
    _, cand = C.candidates([[int(v) for v in row] for row in rows], 64, 2)
    return records, rows, anc, cand


def test_cluster_by_identity(ctx, families):
    """cluster_fasta with min_identity = 0.97, max_distance = 64 against what the yardsticks assemble: candidates, the window of
    every candidate pair, its bytes, the distance, the link; and without the flags the output is today's."""
    from circkit_amd import cluster
    from tests import cluster_ref as C
    from tests import prealign_ref as P
    from tests import sketch_ref as R
    records, rows, anc, cand = families
    n = len(records)
    lengths = [len(r) for r in records]
    w, _, _, bad = P.pairs(rows, anc, lengths, 21, 4, cand)
    assert bad == 0
    cut = [P.window_bytes(records, w[p]) for p in range(len(cand))]
    _, scores, within, _ = D.pairs(records, cut, [(int(a), p) for p, (a, _) in enumerate(cand)], 64)
    assert within >= 120
    q = C.q16(0.97)
    labels = C.link(n, cand, [tuple(int(v) for v in s) for s in scores], (q, 1))[0]
    assert [int(l) for l in labels[:160]] == [4 * (i // 4) for i in range(160)] and [int(l) for l in labels[160:]] == list(range(160, n))
    assert np.array_equal(D.links(scores, q), [C.links(int(s[0]), int(s[1]), q, 1) for s in scores])
    reps = [i for i in range(n) if int(labels[i]) == i]
    fasta = b"".join(b">rec%d planted words\n" % i + records[i] + b"\n" for i in reps)
    table = b"member\trepresentative\n" + b"".join(b"rec%d\trec%d\n" % (i, int(labels[i])) for i in range(n) if int(labels[i]) != i)
    text = _text(records)
    got_fasta, got_table, got_labels = cluster.cluster_fasta(text, min_identity=0.97, max_distance=64)
    assert np.array_equal(got_labels, np.array(labels, dtype=np.uint64))
    assert got_table == table and got_fasta == fasta
    # an identity nobody reaches: every record is its own cluster; a cutoff of 0 links identical records only
    alone = cluster.cluster_fasta(text, min_identity=0.9999, max_distance=64)[2]
    assert np.array_equal(alone, np.arange(n, dtype=np.uint64))
    twice = cluster.cluster_fasta(_text(records[:8] + records[:2]), min_identity=0.5, max_distance=0)[2]
    assert twice.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1]
    # without the flags: today's chain
    match, filled, _ = R.compare_pairs(rows, rows, cand)
    old = C.link(n, cand, list(zip(match.tolist(), filled.tolist())), (C.q16(0.2), 8))[0]
    plain = cluster.cluster_fasta(text)
    assert np.array_equal(plain[2], np.array(old, dtype=np.uint64))
    assert plain[0] == b"".join(b">rec%d planted words\n" % i + records[i] + b"\n" for i in range(n) if int(old[i]) == i)
    with pytest.raises(ValueError):
        cluster.cluster_fasta(text, min_identity=0.9)


def test_prealign_with_distances(ctx, families):
    """prealign_fasta with max_distance = 64: the FASTA is what it is without the flag, and the table's seventh column is the
    yardstick's distance of each written record and its representative."""
    from circkit_amd import prealign
    records, _, _, _ = families
    n = len(records)
    text = _text(records)
    fasta0, table0, labels0 = prealign.prealign_fasta(text)
    fasta, table, labels = prealign.prealign_fasta(text, max_distance=64)
    assert fasta == fasta0 and np.array_equal(labels, labels0)
    written = [b"".join(block.split(b"\n")[1:]) for block in fasta.split(b">")[1:]]
    assert len(written) == n
    exp, _, _, _ = D.pairs(written, None, [(int(labels[i]), i) for i in range(n)], 64)
    rows0, rows = table0.split(b"\n"), table.split(b"\n")
    assert rows[0] == rows0[0] + b"\tdistance" and len(rows) == len(rows0) == n + 2
    for i in range(n):
        assert rows[i + 1] == rows0[i + 1] + (b"\t*" if exp[i] == OVER else b"\t%d" % exp[i]), i
    assert 0 < max(exp[:160]) <= 15 and all(exp[i] == 0 for i in range(0, 160, 4))
    # a cutoff that cuts: the same numbers, `*` beyond it
    low = prealign.prealign_fasta(text, max_distance=5)[1].split(b"\n")
    assert any(r.endswith(b"\t*") for r in low[1:n + 1])
    for i in range(n):
        assert low[i + 1] == rows0[i + 1] + (b"\t*" if exp[i] > 5 else b"\t%d" % exp[i]), i
    assert prealign.prealign_fasta(b"", max_distance=3)[1] == prealign.TITLE[:-1] + b"\tdistance\n"


def test_a_pair_astride_byte_2_to_the_32():
    """One batch round byte 2^32 of a big buffer (tests/test_high_base_gpu.py's buffer, tests/high_base.py's placement): a record
    below the line, one across it and one above it, staged and from global memory."""
    import torch
    from tests import high_base as H
    from tests.test_high_base_gpu import High
    import random
    rng = random.Random(8)
    base = S.rand_seq(rng, 3000)
    seqs = [S.edit(rng, base[:700], 3, 1, 1), base[:700], S.edit(rng, base[:700], 2, 0, 1), base, S.edit(rng, base, 4, 2, 1)]
    data, offs = H.pack(seqs)
    pairs = [(0, 1), (1, 2), (2, 0), (3, 4), (1, 1), (4, 3)]
    exp_d, exp_s, within, _ = D.pairs(seqs, None, pairs, 16)
    assert within == len(pairs) and S.staged(700, 700, 16) and not S.staged(3000, 3000, 16)
    hb = High()
    try:
        for j in (1, 3):
            for mode in H.MODES:
                absolute = H.place(offs, j, mode)
                d_off = hb.put(data, absolute)
                d_pairs = _to(_i32(np.array(pairs, dtype=np.uint32)).reshape(-1))
                d_dist = torch.full((len(pairs),), CANARY32, dtype=torch.int32, device=_dev())
                d_sc = torch.full((2 * len(pairs),), CANARY32, dtype=torch.int32, device=_dev())
                hb.ctx.distance_pairs_device(hb.big, d_off, len(seqs), hb.big, d_off, len(seqs), d_pairs, len(pairs), d_dist, d_sc, max_distance=16)
                assert hb.ctx.distance_status() == (within, 0)
                assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), exp_d), (j, mode)
                assert np.array_equal(d_sc.cpu().numpy().view(np.uint32).reshape(-1, 2), exp_s), (j, mode)
                hb.unchanged((j, mode))
    finally:
        hb.close()
        torch.cuda.empty_cache()
