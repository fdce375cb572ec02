"""GPU: circkit_sketch_anchors_device, circkit_prealign_pairs_device / _status, circkit_prealign_pairs_of_labels_device,
circkit_prealign_batch and the driver circkit_amd/prealign.py against the yardstick tests/prealign_ref.py, exactly: every anchor,
row, count, window, score and total.  The input sets are tests/prealign_sets.py's, the ones the CPU fiber test runs, and the ones
that are too large for the fibers; canaries surround every output."""
import ctypes

import numpy as np
import pytest

from tests import cluster_ref as C
from tests import prealign_ref as P
from tests import prealign_sets as S
from tests import sketch_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY64, CANARY32, CANARY8 = 0x25A5A5A5A5A5A5A5, 0x3F3F3F3F, 0x3F
OK, INVALID_ARG, TOO_LONG = 0, -1, -4
NONE = P.NONE


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


def sketch_status(ctx):
    t, bad = ctypes.c_uint64(0), ctypes.c_uint32(0)
    rc = ctx._lib.circkit_sketch_status(ctx._h, ctypes.byref(t), ctypes.byref(bad))
    return rc, t.value, bad.value


def prealign_status(ctx):
    a, bad = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_prealign_status(ctx._h, ctypes.byref(a), ctypes.byref(bad))
    return rc, a.value, bad.value


class Anchors:
    """A batch on the device and canaries round the rows, the counts and the anchors."""

    def __init__(self, seqs, k, lb, seed, lead):
        import torch
        self.k, self.lb, self.seed = k, lb, seed
        data, offsets = S.csr(seqs, lead)
        self.data, self.offsets = data, offsets
        self.n, self.bins = len(seqs), 1 << lb
        self.d_data = _to(data) if len(data) else torch.zeros(1, dtype=torch.uint8, device=_dev())
        self.d_off = _to(_i64(offsets))
        self.d_rows = torch.full((GUARD + self.n * self.bins + GUARD,), CANARY64, dtype=torch.int64, device=_dev())
        self.d_counts = torch.full((GUARD + self.n + GUARD,), CANARY32, dtype=torch.int32, device=_dev())
        self.d_anc = torch.full((GUARD + self.n * self.bins + GUARD,), CANARY32, dtype=torch.int32, device=_dev())

    def launch(self, ctx, anchors=True, counts=True):
        d_counts = self.d_counts[GUARD:] if counts else None
        if anchors:
            ctx.sketch_anchors_device(self.d_data, self.d_off, self.n, self.d_rows[GUARD:], self.d_anc[GUARD:], d_counts, k=self.k, log2_bins=self.lb, seed=self.seed)
        else:
            ctx.sketch_batch_device(self.d_data, self.d_off, self.n, self.d_rows[GUARD:], d_counts, k=self.k, log2_bins=self.lb, seed=self.seed)

    def result(self):
        """(rows, counts, anchors) after the canary checks."""
        rows, counts, anc = self.d_rows.cpu().numpy().view(np.uint64), self.d_counts.cpu().numpy().view(np.uint32), self.d_anc.cpu().numpy().view(np.uint32)
        w = self.n * self.bins
        assert (rows[:GUARD] == CANARY64).all() and (rows[GUARD + w:] == CANARY64).all(), "rows written outside the n rows"
        assert (counts[:GUARD] == CANARY32).all() and (counts[GUARD + self.n:] == CANARY32).all(), "counts written outside the n"
        assert (anc[:GUARD] == CANARY32).all() and (anc[GUARD + w:] == CANARY32).all(), "anchors written outside the n rows"
        if len(self.data):
            assert np.array_equal(self.d_data.cpu().numpy(), self.data), "the sketch wrote into the payload"
        assert np.array_equal(self.d_off.cpu().numpy().view(np.uint64), self.offsets)
        return (rows[GUARD:GUARD + w].reshape(self.n, self.bins).copy(), counts[GUARD:GUARD + self.n].copy(),
                anc[GUARD:GUARD + w].reshape(self.n, self.bins).copy())


def check_anchors(ctx, name):
    cases = S.anchor_cases()
    case = cases[name] if name in cases else S.anchor_grid_cases()[name]
    exp_rows, exp_counts, exp_anc = S.expected_anchors(name)
    a = Anchors(*case)
    a.launch(ctx)
    rc, valid, bad = sketch_status(ctx)
    rows, counts, anc = a.result()
    assert (rc, valid, bad) == (OK, int(exp_counts.sum()), 0), name
    assert np.array_equal(rows, exp_rows) and np.array_equal(counts, exp_counts), name
    assert np.array_equal(anc, exp_anc), name
    # the same bits a second time, and the rows and counts of the plain sketch on the same ctx
    a.d_anc[GUARD:GUARD + a.n * a.bins] = 0x11111111
    a.launch(ctx)
    assert sketch_status(ctx)[0] == OK
    rows2, counts2, anc2 = a.result()
    assert np.array_equal(rows2, rows) and np.array_equal(counts2, counts) and np.array_equal(anc2, anc), name
    a.d_rows[GUARD:GUARD + a.n * a.bins] = 0
    a.d_counts[GUARD:GUARD + a.n] = 0
    a.launch(ctx, anchors=False)
    assert sketch_status(ctx) == (OK, int(exp_counts.sum()), 0)
    rows3, counts3, anc3 = a.result()
    assert np.array_equal(rows3, rows) and np.array_equal(counts3, counts) and np.array_equal(anc3, anc), name
    return a


@pytest.mark.parametrize("name", sorted(S.anchor_cases()))
def test_anchors(ctx, name):
    check_anchors(ctx, name)


@pytest.mark.parametrize("name", ["past_short_grid", "past_long_grid"])
def test_anchors_one_record_past_each_grid(ctx, name):
    check_anchors(ctx, name)


def test_anchors_without_counts_and_without_records(ctx):
    import torch
    a = Anchors(*S.anchor_cases()["lengths"])
    a.launch(ctx, counts=False)
    assert sketch_status(ctx)[0] == OK
    rows, counts, anc = a.result()
    assert (counts == CANARY32).all() and np.array_equal(anc, S.expected_anchors("lengths")[2]) and np.array_equal(rows, S.expected_anchors("lengths")[0])
    ctx.sketch_anchors_device(None, None, 0, None, None, None, k=8, log2_bins=4)
    assert sketch_status(ctx) == (OK, 0, 0)
    # a record of 2^31 symbols (by the offsets alone: never dereferenced) gets an empty row and NONE anchors, and is counted
    seqs = [b"ACGTACGTTGCA", b"GATTACAGATTACA"]
    data, _ = S.csr(seqs)
    offs = np.array([0, 12, 26, 26 + 2 ** 31], dtype=np.uint64)              # (the last record: nothing lies behind it)
    d_data, d_off = _to(data), _to(_i64(offs))
    d_rows = torch.zeros(3 * 16, dtype=torch.int64, device=_dev())
    d_anc = torch.zeros(3 * 16, dtype=torch.int32, device=_dev())
    ctx.sketch_anchors_device(d_data, d_off, 3, d_rows, d_anc, None, k=4, log2_bins=4)
    rc, _, bad = sketch_status(ctx)
    assert (rc, bad) == (TOO_LONG, 1)
    anc = d_anc.cpu().numpy().view(np.uint32).reshape(3, 16)
    assert (anc[2] == NONE).all() and (d_rows.cpu().numpy().view(np.uint64).reshape(3, 16)[2] == P.EMPTY).all()
    for i in range(2):
        assert np.array_equal(anc[i], np.array(P.anchors(seqs[i], 4, 4)[2], dtype=np.uint32))


class Votes:
    """Rows, anchors, offsets and pairs on the device and canaries round the windows and the scores."""

    def __init__(self, rows, anc, lengths, k, mv, pairs):
        import torch
        self.rows, self.anc = np.ascontiguousarray(rows, dtype=np.uint64), np.ascontiguousarray(anc, dtype=np.uint32)
        self.n, self.lb, self.k, self.mv = len(self.rows), self.rows.shape[1].bit_length() - 1, k, mv
        self.pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64).astype(np.uint32)).reshape(-1, 2)
        self.m = len(self.pairs)
        self.d_rows = _to(_i64(self.rows).reshape(-1)) if self.n else None
        self.d_anc = _to(_i32(self.anc).reshape(-1)) if self.n else None
        self.d_off = _to(_i64(S.offsets_of(lengths))) if self.n else None
        self.d_pairs = _to(_i32(self.pairs).reshape(-1)) if self.m else None
        self.d_win = torch.full((24 * GUARD + 24 * self.m + 24 * GUARD,), CANARY8, dtype=torch.uint8, device=_dev())
        self.d_scores = torch.full((2 * GUARD + 2 * self.m + 2 * GUARD,), CANARY32, dtype=torch.int32, device=_dev())

    def launch(self, ctx):
        ctx.prealign_pairs_device(self.d_rows, self.d_anc, self.d_off, self.n, self.d_pairs, self.m, self.d_win[24 * GUARD:], self.d_scores[2 * GUARD:],
                                  k=self.k, log2_bins=self.lb, min_votes=self.mv)

    def result(self):
        win, sc = self.d_win.cpu().numpy(), self.d_scores.cpu().numpy().view(np.uint32)
        assert (win[:24 * GUARD] == CANARY8).all() and (win[24 * GUARD + 24 * self.m:] == CANARY8).all(), "windows written outside the n_pairs"
        assert (sc[:2 * GUARD] == CANARY32).all() and (sc[2 * GUARD + 2 * self.m:] == CANARY32).all(), "scores written outside the n_pairs"
        if self.n:
            assert np.array_equal(self.d_rows.cpu().numpy().view(np.uint64).reshape(self.rows.shape), self.rows)
            assert np.array_equal(self.d_anc.cpu().numpy().view(np.uint32).reshape(self.anc.shape), self.anc)
        if self.m:
            assert np.array_equal(self.d_pairs.cpu().numpy().view(np.uint32).reshape(-1, 2), self.pairs)
        return (win[24 * GUARD:24 * GUARD + 24 * self.m].copy().view(P.WINDOW_DTYPE), sc[2 * GUARD:2 * GUARD + 2 * self.m].reshape(-1, 2).copy())


def check_votes(ctx, name):
    case = S.past_the_pairs_grid() if name == "past_the_pairs_grid" else S.vote_cases()[name]
    w, sc, al, bad = S.expected_votes(name)
    v = Votes(*case)
    v.launch(ctx)
    rc, got_al, got_bad = prealign_status(ctx)
    got_w, got_sc = v.result()
    assert (rc, got_al, got_bad) == (INVALID_ARG if bad else OK, al, bad), name
    assert np.array_equal(got_w, w), name
    assert np.array_equal(got_sc, sc), name
    return v


@pytest.mark.parametrize("name", sorted(S.vote_cases()) + ["past_the_pairs_grid"])
def test_votes(ctx, name):
    check_votes(ctx, name)


@pytest.mark.parametrize("name", sorted(S.label_cases()))
def test_pairs_of_labels(ctx, name):
    import torch
    labels = S.label_cases()[name]
    n = len(labels)
    d_labels = _to(_i64(labels)) if n else None
    d_pairs = torch.full((2 * GUARD + 2 * n + 2 * GUARD,), CANARY32, dtype=torch.int32, device=_dev())
    ctx.prealign_pairs_of_labels_device(d_labels, n, d_pairs[2 * GUARD:])
    ctx.synchronize()
    got = d_pairs.cpu().numpy().view(np.uint32)
    assert (got[:2 * GUARD] == CANARY32).all() and (got[2 * GUARD + 2 * n:] == CANARY32).all()
    exp = np.empty((n, 2), dtype=np.uint32)                  # the yardstick's rule as array expressions (held against it below)
    exp[:, 0] = np.where(labels >> np.uint64(32), np.uint64(NONE), labels).astype(np.uint32)
    exp[:, 1] = np.arange(n, dtype=np.uint32)
    assert np.array_equal(exp[:1000], P.pairs_of_labels(labels[:1000]))
    assert np.array_equal(got[2 * GUARD:2 * GUARD + 2 * n].reshape(-1, 2), exp)
    if name == "wide":                                        # the pairs call counts what the labels call marked
        rows, anc, lengths = S.vote_cases()["rotations"][:3]
        v = Votes(rows[:5], anc[:5], lengths[:5], 8, 4, exp)
        v.launch(ctx)
        w, sc, al, bad = P.pairs(rows[:5], anc[:5], lengths[:5], 8, 4, exp)
        assert bad == 3 and prealign_status(ctx) == (INVALID_ARG, al, bad)
        assert np.array_equal(v.result()[0], w)


def test_the_statuses_are_their_own(ctx):
    """A plain sketch, a compare and a cluster call between a call and its status change neither the sketch's nor prealign's totals."""
    import torch
    a = check_anchors(ctx, "lengths")
    valid = int(S.expected_anchors("lengths")[1].sum())
    v = check_votes(ctx, "invalid")
    mine = (INVALID_ARG,) + tuple(S.expected_votes("invalid")[2:])
    assert mine[2] == 5
    assert sketch_status(ctx) == (OK, valid, 0)              # prealign in between
    other = Anchors(*S.anchor_cases()["k4"])
    other.launch(ctx, anchors=False)                          # a plain sketch in between: the sketch's totals are the most recent sketch's
    assert prealign_status(ctx) == mine
    assert sketch_status(ctx)[1] == int(S.expected_anchors("k4")[1].sum())
    rows = S.vote_cases()["rotations"][0]
    n = len(rows)
    d_rows = _to(_i64(rows).reshape(-1))
    d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=_dev())
    d_pairs = torch.empty(2 * n * 16, dtype=torch.int32, device=_dev())
    d_scores = torch.empty(2 * n * 16, dtype=torch.int32, device=_dev())
    d_labels = torch.empty(n, dtype=torch.int64, device=_dev())
    ctx.cluster_candidates_device(d_rows, n, 5, d_pair_off, d_pairs, n * 16, n_bands=16, band_bins=2)
    m = ctx.cluster_candidates_status()
    ctx.sketch_compare_device(d_rows, n, d_rows, n, 5, d_pairs, m, d_scores)
    ctx.cluster_link_device(n, d_pairs, d_scores, m, d_labels, n_bands=16, band_bins=2)
    assert ctx.cluster_link_status()[0] == 1                  # every rotation and strand of one record: one cluster
    assert prealign_status(ctx) == mine
    check_votes(ctx, "self_pairs")
    assert prealign_status(ctx) == (OK, 9, 0)
    del a, v


def test_argument_errors_change_nothing(ctx):
    import torch
    from circkit_amd import api
    v = check_votes(ctx, "rotations")
    before = prealign_status(ctx)
    win0, sc0 = v.d_win.clone(), v.d_scores.clone()
    lib, h = ctx._lib, ctx._h
    W, SC = v.d_win[24 * GUARD:], v.d_scores[2 * GUARD:]

    def call(p=None, rows=v.d_rows, anc=v.d_anc, off=v.d_off, n=v.n, pairs=v.d_pairs, m=v.m, win=W, sc=SC):
        p = p or api.prealign_params(k=8, log2_bins=5, min_votes=4)
        return lib.circkit_prealign_pairs_device(h, api._ptr(rows), api._ptr(anc), api._ptr(off), n, ctypes.byref(p), api._ptr(pairs), m, api._ptr(win), api._ptr(sc))

    bad_params = [api.prealign_params(k=3, log2_bins=5), api.prealign_params(k=33, log2_bins=5), api.prealign_params(k=8, log2_bins=3),
                  api.prealign_params(k=8, log2_bins=11), api.prealign_params(k=8, log2_bins=5, min_votes=0)]
    r = api.prealign_params(k=8, log2_bins=5)
    r.reserved = 1
    for p in bad_params + [r]:
        assert call(p=p) == INVALID_ARG
    assert lib.circkit_prealign_pairs_device(h, api._ptr(v.d_rows), api._ptr(v.d_anc), api._ptr(v.d_off), v.n, None, api._ptr(v.d_pairs), v.m, api._ptr(W), api._ptr(SC)) == INVALID_ARG
    for kw in (dict(rows=None), dict(anc=None), dict(off=None), dict(pairs=None), dict(win=None), dict(sc=None), dict(n=2 ** 32)):
        assert call(**kw) == INVALID_ARG, kw
    # an output over an input, or over the other output
    for kw in (dict(win=v.d_rows), dict(sc=v.d_rows), dict(win=v.d_anc), dict(sc=v.d_pairs), dict(win=v.d_off), dict(sc=W), dict(win=SC)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(win=v.d_win[24 * GUARD + 4:]) == INVALID_ARG                              # the windows are 8-byte aligned
    assert prealign_status(ctx) == before
    assert torch.equal(v.d_win, win0) and torch.equal(v.d_scores, sc0)
    v.result()
    # the anchors call: a null or overlapping anchors buffer, as for the other outputs
    a = Anchors(*S.anchor_cases()["k4"])
    a.launch(ctx)
    status = sketch_status(ctx)
    rows0, counts0, anc0 = a.d_rows.clone(), a.d_counts.clone(), a.d_anc.clone()
    sp = api.sketch_params(k=4, log2_bins=4)
    R_, C_, A_ = a.d_rows[GUARD:], a.d_counts[GUARD:], a.d_anc[GUARD:]

    def sk(p=sp, data=a.d_data, off=a.d_off, rows=R_, counts=C_, anc=A_):
        return lib.circkit_sketch_anchors_device(h, api._ptr(data), api._ptr(off), a.n, ctypes.byref(p), api._ptr(rows), api._ptr(counts), api._ptr(anc))

    for kw in (dict(anc=None), dict(rows=None), dict(data=None), dict(off=None), dict(anc=R_), dict(anc=C_), dict(anc=a.d_off), dict(counts=A_),
               dict(p=api.sketch_params(k=3, log2_bins=4)), dict(p=api.sketch_params(k=4, log2_bins=11))):
        assert sk(**kw) == INVALID_ARG, kw
    assert sketch_status(ctx) == status
    assert torch.equal(a.d_rows, rows0) and torch.equal(a.d_counts, counts0) and torch.equal(a.d_anc, anc0)
    d_pairs = torch.full((8,), CANARY32, dtype=torch.int32, device=_dev())
    d_labels = torch.zeros(4, dtype=torch.int64, device=_dev())
    assert lib.circkit_prealign_pairs_of_labels_device(h, None, 4, api._ptr(d_pairs)) == INVALID_ARG
    assert lib.circkit_prealign_pairs_of_labels_device(h, api._ptr(d_labels), 4, None) == INVALID_ARG
    assert lib.circkit_prealign_pairs_of_labels_device(h, api._ptr(d_labels), 2 ** 32, api._ptr(d_pairs)) == INVALID_ARG
    assert lib.circkit_prealign_pairs_of_labels_device(h, api._ptr(d_labels), 4, api._ptr(d_labels)) == INVALID_ARG
    ctx.synchronize()
    assert (d_pairs.cpu().numpy().view(np.uint32) == CANARY32).all()
    # the host form: refused from the offsets alone
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    pairs = np.array([[0, 1]], dtype=np.uint32)
    win, sc = np.full(1, 7, dtype=np.uint64).repeat(3), np.full(2, 7, dtype=np.uint32)
    for offs, code in (([0, 10, 10 + 2 ** 31], TOO_LONG), ([1, 10, 10], INVALID_ARG), ([0, 10, 4], INVALID_ARG)):
        offs = np.array(offs, dtype=np.uint64)
        assert lib.circkit_prealign_batch(h, api._ptr(data), api._ptr(offs), 2, ctypes.byref(sp), api._ptr(pairs), 1, 4, api._ptr(win), api._ptr(sc)) == code
    offs = np.array([0, 5, 10], dtype=np.uint64)
    assert lib.circkit_prealign_batch(h, api._ptr(data), api._ptr(offs), 2, ctypes.byref(sp), api._ptr(pairs), 1, 0, api._ptr(win), api._ptr(sc)) == INVALID_ARG
    assert (win == 7).all() and (sc == 7).all()


def test_the_planted_set_through_the_host_form(ctx):
    import circkit_amd
    records, plants = S.planted()
    pairs = [(fi, ci) for fi, ci, _, _, _ in plants] + [(a, b) for a in range(0, 160, 4) for b in range(4, 160, 36)]
    rows, _, anc = P.anchors_batch(records, 21, 8)
    lengths = [len(r) for r in records]
    w, sc, al, bad = P.pairs(rows, anc, lengths, 21, 4, pairs)
    got_w, got_sc = circkit_amd.prealign_batch(records, pairs)
    assert got_w.dtype == P.WINDOW_DTYPE and np.array_equal(got_w, w) and np.array_equal(got_sc, sc)
    for at, (fi, ci, r, s, subs) in enumerate(plants):
        assert (int(got_w[at]["start"]), int(got_w[at]["strand"])) == S.planted_window(lengths[fi], r, s)
    # the windows go to windows_gather as they are: every copy comes back as its founder but for the planted substitutions
    data, offsets = S.csr(records)
    out, out_off = circkit_amd.default_context().windows_gather(data, offsets, got_w[:len(plants)])
    out = out.tobytes()
    for at, (fi, ci, r, s, subs) in enumerate(plants):
        cut = out[int(out_off[at]):int(out_off[at + 1])]
        assert [p for p in range(lengths[fi]) if cut[p] != records[fi][p]] == subs
    rows_g, counts_g, anc_g = circkit_amd.sketch_anchors(records[:8])
    assert np.array_equal(rows_g, rows[:8]) and np.array_equal(anc_g, anc[:8]) and counts_g.tolist() == lengths[:8]
    none = circkit_amd.prealign_batch([], [])
    assert len(none[0]) == 0 and none[1].shape == (0, 2)
    with pytest.raises(circkit_amd.CirckitError):
        circkit_amd.prealign_batch(records[:4], [(0, 4)])


def _planted_text(records):
    return b"".join(b">rec%d planted words\n" % i + r[:70] + b"\n" + r[70:] + b"\n" for i, r in enumerate(records))


def test_text_to_text(ctx):
    """prealign_fasta against the file the yardsticks assemble: sketch and anchors, candidates, compare, link, the pairs of the
    labels, the votes, the windows' bytes, the heads; and the table."""
    from circkit_amd import prealign
    records, plants = S.planted()
    n = len(records)
    rows, _, anc = P.anchors_batch(records, 21, 8)
    _, cand = C.candidates([[int(v) for v in row] for row in rows], 64, 2)
    match, filled, _ = R.compare_pairs(rows, rows, cand)
    labels = C.link(n, cand, list(zip(match.tolist(), filled.tolist())), (C.q16(0.2), 8))[0]
    assert [int(l) for l in labels] == [4 * (i // 4) for i in range(n)]                  # the families are the clusters
    w, sc, al, bad = P.pairs(rows, anc, [len(r) for r in records], 21, 4, P.pairs_of_labels(labels))
    assert al == n and bad == 0
    fasta = b"".join(b">rec%d planted words\n" % i + P.window_bytes(records, w[i]) + b"\n" for i in range(n))
    table = prealign.TITLE + b"".join(b"rec%d\trec%d\t%d\t%d\t%d\t%d\n" % (i, int(labels[i]), w[i]["strand"], w[i]["start"], sc[i][0], sc[i][1])
                                      for i in range(n))
    got_fasta, got_table, got_labels = prealign.prealign_fasta(_planted_text(records))
    assert np.array_equal(got_labels, np.array(labels, dtype=np.uint64))
    assert got_table == table
    assert got_fasta == fasta
    # a threshold nobody reaches: every record comes out as it went in
    plain, table2, _ = prealign.prealign_fasta(_planted_text(records), min_votes=257)
    assert plain == b"".join(b">rec%d planted words\n" % i + r + b"\n" for i, r in enumerate(records))
    empty = prealign.prealign_fasta(b"")
    assert empty[:2] == (b"", prealign.TITLE) and len(empty[2]) == 0
    with pytest.raises(ValueError):
        prealign.prealign_fasta(b"ACGT\n>x\nACGT\n")


def test_invariance_under_rotation_and_strand(ctx):
    """Where the yardstick says the votes are unanimous (votes == matches, before and after), the gathered output does not depend on
    how the members were cut or read: rotate_batch / revcomp_batch over the members first, the same bytes afterwards."""
    import circkit_amd
    records, plants = S.planted()
    n = len(records)
    pairs = [(4 * (i // 4), i) for i in range(n)]
    data, offsets = S.csr(records)
    members = np.array([i % 4 != 0 for i in range(n)])

    def moved(kind):
        if kind == "rotate":
            out, off = circkit_amd.rotate_batch(data, offsets, bases=37)
        else:
            out, off = circkit_amd.revcomp_batch(data, offsets)
        out = out.tobytes()
        return [out[int(off[i]):int(off[i + 1])] if members[i] else records[i] for i in range(n)]

    def unanimous(seqs):
        rows, _, anc = P.anchors_batch(seqs, 21, 8)
        _, sc, _, _ = P.pairs(rows, anc, [len(s) for s in seqs], 21, 4, pairs)
        return (sc[:, 0] == sc[:, 1]) & (sc[:, 0] >= 4)

    def gathered(seqs):
        w, _ = circkit_amd.prealign_batch(seqs, pairs)
        d, o = S.csr(seqs)
        out, off = circkit_amd.default_context().windows_gather(d, o, w)
        out = out.tobytes()
        return [out[int(off[i]):int(off[i + 1])] for i in range(n)]

    base_ok, base = unanimous(records), gathered(records)
    for kind in ("rotate", "revcomp"):
        seqs = moved(kind)
        assert seqs[1] != records[1]
        ok = base_ok & unanimous(seqs)
        assert ok.sum() > n // 2
        got = gathered(seqs)
        for i in np.flatnonzero(ok):
            assert got[i] == base[i], (kind, int(i))
