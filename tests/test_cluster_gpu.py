"""GPU: circkit_cluster_candidates_device / _status, circkit_cluster_link_device / _status, circkit_cluster_batch and the driver
circkit_amd/cluster.py against the yardstick tests/cluster_ref.py, exactly: every offset, pair, label and total.  The input sets
are tests/cluster_sets.py's, the ones the CPU fiber test runs; canaries surround the offsets, the pairs and the labels."""
import ctypes

import numpy as np
import pytest

from tests import cluster_ref as C
from tests import cluster_sets as S
from tests import sketch_ref as R
from tests import sketch_sets as SS

pytestmark = pytest.mark.gpu

GUARD = 64
OFF_CANARY, PAIR_CANARY = 0x25A5A5A5A5A5A5A5, 0x3F3F3F3F
OK, INVALID_ARG, TOO_LONG, OOM = 0, -1, -4, -5


def _dev():
    import torch
    return torch.device("cuda", 0)


def _to(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


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


def candidates_status(ctx):
    t = ctypes.c_uint64(0)
    rc = ctx._lib.circkit_cluster_candidates_status(ctx._h, ctypes.byref(t))
    return rc, t.value


def link_status(ctx):
    a, b, bad = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = ctx._lib.circkit_cluster_link_status(ctx._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(bad))
    return rc, a.value, b.value, bad.value


class Candidates:
    """The rows on the device and canaries round the offsets and the pair buffer of `capacity` pairs."""

    def __init__(self, rows, capacity):
        import torch
        self.rows = np.ascontiguousarray(rows, dtype=np.uint64)
        self.n, self.log2_bins, self.capacity = len(self.rows), self.rows.shape[1].bit_length() - 1, capacity
        self.d_rows = _to(self.rows.view(np.int64).reshape(-1)) if self.n else torch.zeros(1, dtype=torch.int64, device=_dev())
        self.d_off = torch.full((GUARD + self.n + 1 + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
        self.d_pairs = torch.full((2 * GUARD + 2 * capacity + 2 * GUARD,), PAIR_CANARY, dtype=torch.int32, device=_dev())

    def launch(self, ctx, n_bands, band_bins):
        ctx.cluster_candidates_device(self.d_rows, self.n, self.log2_bins, self.d_off[GUARD:], self.d_pairs[2 * GUARD:], self.capacity,
                                      n_bands=n_bands, band_bins=band_bins)

    def result(self):
        """(offsets, pair buffer (capacity, 2)) after the canary checks."""
        off, pairs = self.d_off.cpu().numpy().view(np.uint64), self.d_pairs.cpu().numpy().view(np.uint32)
        assert (off[:GUARD] == OFF_CANARY).all() and (off[GUARD + self.n + 1:] == OFF_CANARY).all(), "offsets written outside the n + 1"
        assert (pairs[:2 * GUARD] == PAIR_CANARY).all() and (pairs[2 * GUARD + 2 * self.capacity:] == PAIR_CANARY).all(), "pairs written past the capacity"
        if self.n:
            assert np.array_equal(self.d_rows.cpu().numpy().view(np.uint64).reshape(self.rows.shape), self.rows), "the candidates wrote into the rows"
        return off[GUARD:GUARD + self.n + 1].copy(), pairs[2 * GUARD:2 * GUARD + 2 * self.capacity].reshape(-1, 2).copy()


def check_candidates(ctx, name, capacity=None):
    rows, nb, bb = S.past_the_emit_grid() if name == "past_the_emit_grid" else S.candidate_cases()[name]
    exp_off, exp_pairs = S.expected_candidates(name)
    cap = len(rows) * nb if capacity is None else capacity
    c = Candidates(rows, cap)
    c.launch(ctx, nb, bb)
    rc, total = candidates_status(ctx)
    off, pairs = c.result()
    assert (rc, total) == (OOM if len(exp_pairs) > cap else OK, len(exp_pairs)), (name, rc, total)
    assert np.array_equal(off, exp_off), name
    assert np.array_equal(pairs, S.pair_buffer(exp_off, exp_pairs, cap, PAIR_CANARY)), name
    return c


def run_link(ctx, n, pairs, scores, params):
    """(labels, rc, clusters, linked, invalid); canaries round the labels."""
    import torch
    pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
    scores = np.ascontiguousarray(scores, dtype=np.uint32).reshape(-1, 2)
    m = len(pairs)
    d_pairs, d_scores = (_to(_i32(pairs)), _to(_i32(scores))) if m else (None, None)
    d_labels = torch.full((GUARD + n + GUARD,), OFF_CANARY, dtype=torch.int64, device=_dev())
    from circkit_amd import api
    p = api.cluster_params()
    p.min_similarity_q16, p.min_filled = params
    ctx.cluster_link_device(n, d_pairs, d_scores, m, d_labels[GUARD:], params=p)
    rc, clusters, linked, invalid = link_status(ctx)
    labels = d_labels.cpu().numpy().view(np.uint64)
    assert (labels[:GUARD] == OFF_CANARY).all() and (labels[GUARD + n:] == OFF_CANARY).all(), "labels written outside the n records'"
    if m:
        assert np.array_equal(d_pairs.cpu().numpy().view(np.uint32), pairs) and np.array_equal(d_scores.cpu().numpy().view(np.uint32), scores)
    return labels[GUARD:GUARD + n].copy(), rc, clusters, linked, invalid


# ---- 1. candidates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.candidate_cases()))
def test_candidates(ctx, name):
    check_candidates(ctx, name)


def test_one_record_past_the_grids(ctx):
    """One record past the count and write kernels' grid; at 64 bands the keys kernel's lanes make a second trip too."""
    c = S.constants()
    rows, nb, _ = S.past_the_emit_grid()
    assert len(rows) == c["EMIT_MAX_GRID"] * c["EMIT_WAVES"] + 1 and len(rows) * nb > c["KEYS_MAX_GRID"] * c["KEYS_WG"]
    check_candidates(ctx, "past_the_emit_grid")
    assert S.expected_candidates("past_the_emit_grid")[0][-1] > S.expected_candidates("past_the_emit_grid")[0][-2]     # the last record proposes


def test_the_capacity_rule(ctx):
    """Exactly the total, one less, the middle, 0: the offsets and the total are exact, a record that does not fit is not written,
    the status is OOM."""
    total = len(S.expected_candidates("several_earlier")[1])
    for cap in (total, total - 1, total // 2, 0):
        check_candidates(ctx, "several_earlier", capacity=cap)
    total = len(S.expected_candidates("identical_x1000")[1])
    for cap in (total, total - 1, 0):
        check_candidates(ctx, "identical_x1000", capacity=cap)


def test_no_records(ctx):
    from circkit_amd import api
    check_candidates(ctx, "records_0")
    off = _to(np.full(1, 7, dtype=np.int64))
    assert ctx._lib.circkit_cluster_candidates_device(ctx._h, None, 0, 8, ctypes.byref(api.cluster_params()), api._ptr(off), None, 0) == OK
    assert candidates_status(ctx) == (OK, 0) and off.cpu().numpy().tolist() == [0]
    labels, rc, clusters, linked, invalid = run_link(ctx, 0, [], [], S.DEFAULT)
    assert (rc, clusters, linked, invalid) == (OK, 0, 0, 0)
    assert ctx._lib.circkit_cluster_link_device(ctx._h, 0, None, None, 0, ctypes.byref(api.cluster_params()), None) == OK
    assert link_status(ctx) == (OK, 0, 0, 0)


# ---- 2. link -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.link_cases()))
def test_link(ctx, name):
    n, pairs, scores, params = S.link_cases()[name]
    exp_labels, clusters, linked, invalid = S.expected_link(name)
    got = run_link(ctx, n, pairs, scores, params)
    assert np.array_equal(got[0], exp_labels), name
    assert got[1:] == (INVALID_ARG if invalid else OK, clusters, linked, invalid), name


@pytest.mark.parametrize("name", S.CONTENTION)
def test_contention(ctx, name):
    """Shapes in which many lanes change the same roots at once, at full size, twice: the labels are the yardstick's both times."""
    n, pairs, scores, params = S.contention(name)
    exp_labels, clusters, linked, invalid = S.expected_link(name)
    assert len(pairs) >= {"star": 100_000, "path": 49_999, "clique": 44_850, "two_joined_last": 39_999, "many_components": 98_000}[name]
    first = run_link(ctx, n, pairs, scores, params)
    second = run_link(ctx, n, pairs, scores, params)
    for got in (first, second):
        assert np.array_equal(got[0], exp_labels), name
        assert got[1:] == (OK, clusters, linked, 0), name


def test_one_pair_and_one_record_past_the_link_grids(ctx):
    """One pair past the link kernel's grid and one record past the init and flatten kernels': the last pair links the last
    record, and one in sixteen of the others links."""
    c = S.constants()
    m, n = c["LINK_MAX_GRID"] * c["LINK_WG"] + 1, c["FLATTEN_MAX_GRID"] * c["LINK_WG"] + 1
    p = np.arange(m, dtype=np.uint64)
    pairs = np.stack([p % np.uint64(n - 1), (p * np.uint64(7) + np.uint64(1)) % np.uint64(n - 1)], axis=1).astype(np.uint32)
    pairs[-1] = (n - 1, 3)
    scores = np.where((p % np.uint64(16) == 0)[:, None], np.array(S.PASS, dtype=np.uint32), np.array((1, 100), dtype=np.uint32))
    scores[-1] = S.PASS
    labels, n_clusters, n_linked, n_invalid = C.link(n, pairs.tolist(), scores.tolist(), S.DEFAULT)
    got = run_link(ctx, n, pairs, scores, S.DEFAULT)
    assert labels[n - 1] < n - 1 and n_linked > m // 17
    assert np.array_equal(got[0], np.array(labels, dtype=np.uint64)) and got[1:] == (OK, n_clusters, n_linked, 0)


# ---- 3. statuses and argument errors ---------------------------------------------------------------------------------------------
def test_each_status_answers_for_its_own_kind(ctx):
    """A sketch and a uniq compact between a candidates call, a link and their statuses."""
    import torch
    rows, nb, bb = S.candidate_cases()["several_earlier"]
    c = Candidates(rows, 3)
    c.launch(ctx, nb, bb)
    n, pairs, scores, params = S.link_cases()["invalid_among_valid"]
    d_pairs, d_scores, d_labels = _to(_i32(np.array(pairs, dtype=np.uint32))), _to(_i32(np.array(scores, dtype=np.uint32))), torch.zeros(n, dtype=torch.int64, device=_dev())
    ctx.cluster_link_device(n, d_pairs, d_scores, len(pairs), d_labels)
    # another unit's work behind both
    recs = (b"ACGTTGCAAC" * 5, b"GATTACA" * 9)
    data, offs = SS.pack(recs)
    d_bytes, d_offs = _to(data), _to(_i64(offs))
    d_sk = torch.zeros(2 * 16, dtype=torch.int64, device=_dev())
    ctx.sketch_batch_device(d_bytes, d_offs, 2, d_sk, k=5, log2_bins=4)
    d_fs = _to(_i64(np.array([0, 0], dtype=np.uint64)))
    d_out, d_out_off, d_out_src = torch.zeros(len(data), dtype=torch.uint8, device=_dev()), torch.zeros(3, dtype=torch.int64, device=_dev()), torch.zeros(2, dtype=torch.int64, device=_dev())
    ctx.uniq_compact_device(d_bytes, d_offs, 2, d_fs, d_out, d_out_off, d_out_src)
    assert ctx.uniq_compact_status() == (1, 50)
    total = len(S.expected_candidates("several_earlier")[1])
    assert candidates_status(ctx) == (OOM, total)
    exp = S.expected_link("invalid_among_valid")
    assert link_status(ctx) == (INVALID_ARG, *exp[1:])
    assert ctx.sketch_status()[0] == int(SS.expected(recs, 5, 4)[1].sum())
    assert candidates_status(ctx) == (OOM, total) and link_status(ctx) == (INVALID_ARG, *exp[1:])
    assert np.array_equal(d_labels.cpu().numpy().view(np.uint64), exp[0])


def test_argument_errors_enqueue_nothing(ctx):
    import torch
    from circkit_amd import api
    c = check_candidates(ctx, "several_earlier")
    rows, nb, bb = S.candidate_cases()["several_earlier"]
    n, pairs, scores, params = S.link_cases()["both_orientations"]
    d_pairs, d_scores = _to(_i32(np.array(pairs, dtype=np.uint32))), _to(_i32(np.array(scores, dtype=np.uint32)))
    d_labels = torch.full((n,), 77, dtype=torch.int64, device=_dev())
    ctx.cluster_link_device(n, d_pairs, d_scores, len(pairs), d_labels)
    before = (candidates_status(ctx), link_status(ctx))
    out_before, labels_before = c.result(), d_labels.cpu().numpy().copy()
    lib, h = ctx._lib, ctx._h
    good = api.cluster_params(n_bands=nb, band_bins=bb)

    def cand(p=good, d_rows=c.d_rows, n_records=c.n, log2_bins=c.log2_bins, d_off=c.d_off[GUARD:], d_pairs=c.d_pairs[2 * GUARD:], cap=c.capacity, by_ref=True):
        return lib.circkit_cluster_candidates_device(h, api._ptr(d_rows), n_records, log2_bins, ctypes.byref(p) if by_ref else None, api._ptr(d_off),
                                                     api._ptr(d_pairs), cap)

    def link(p=good, n_records=n, pairs=d_pairs, sc=d_scores, m=len(pairs), labels=d_labels, by_ref=True):
        return lib.circkit_cluster_link_device(h, n_records, api._ptr(pairs), api._ptr(sc), m, ctypes.byref(p) if by_ref else None, api._ptr(labels))

    bad_params = [dict(n_bands=0), dict(n_bands=65), dict(band_bins=0), dict(band_bins=17), dict(min_filled=0)]
    for kw in bad_params:
        p = api.cluster_params(**{**dict(n_bands=nb, band_bins=bb), **kw})
        assert cand(p) == INVALID_ARG and link(p) == INVALID_ARG, kw
    p = api.cluster_params(n_bands=nb, band_bins=bb)
    p.min_similarity_q16 = 65537
    assert cand(p) == INVALID_ARG and link(p) == INVALID_ARG
    for r in ((1, 0), (0, 1)):
        p = api.cluster_params(n_bands=nb, band_bins=bb)
        p.reserved[0], p.reserved[1] = r
        assert cand(p) == INVALID_ARG and link(p) == INVALID_ARG
    assert cand(by_ref=False) == INVALID_ARG and link(by_ref=False) == INVALID_ARG
    assert cand(api.cluster_params(n_bands=9, band_bins=2)) == INVALID_ARG            # 18 bins of 16
    assert cand(api.cluster_params(n_bands=2, band_bins=9)) == INVALID_ARG
    assert cand(log2_bins=3) == INVALID_ARG and cand(log2_bins=11) == INVALID_ARG
    assert cand(d_rows=None) == INVALID_ARG and cand(d_off=None) == INVALID_ARG and cand(d_pairs=None) == INVALID_ARG
    assert cand(n_records=2 ** 32) == INVALID_ARG and cand(n_records=(2 ** 32 - 1) // nb + 1) == INVALID_ARG
    assert cand(api.cluster_params(n_bands=1, band_bins=1), n_records=2 ** 32 - 1) == INVALID_ARG
    # outputs over the input or each other
    assert cand(d_off=c.d_rows[1:]) == INVALID_ARG and cand(d_pairs=c.d_rows.view(torch.int32)[2:]) == INVALID_ARG
    assert cand(d_pairs=c.d_off[GUARD:].view(torch.int32)[2:]) == INVALID_ARG
    assert link(pairs=None) == INVALID_ARG and link(sc=None) == INVALID_ARG and link(labels=None) == INVALID_ARG
    assert link(n_records=2 ** 32) == INVALID_ARG
    assert link(labels=d_pairs.view(torch.int64)) == INVALID_ARG and link(labels=d_scores.view(torch.int64)[1:]) == INVALID_ARG
    assert lib.circkit_cluster_candidates_device(None, None, 0, 8, ctypes.byref(good), None, None, 0) == INVALID_ARG
    # nothing ran: the statuses and every buffer are as they were
    assert (candidates_status(ctx), link_status(ctx)) == before
    out_after = c.result()
    assert np.array_equal(out_after[0], out_before[0]) and np.array_equal(out_after[1], out_before[1])
    assert np.array_equal(d_labels.cpu().numpy(), labels_before)
    assert cand() == OK and link() == OK and (candidates_status(ctx), link_status(ctx)) == before


# ---- 4. the chain, the host form, the driver -----------------------------------------------------------------------------------------
def family_text(records):
    return b"".join(b">rec%d family words\n" % i + b"\n".join(s[j:j + 70] for j in range(0, len(s), 70)).lower() + b"\n" for i, s in enumerate(records))


def test_text_to_clusters_to_text(ctx):
    """fasta_parse_gpu -> sketch -> candidates -> compare -> link -> uniq_compact -> fasta_write on the planted set without the
    batch leaving the device, every stage against the yardstick, the file against the yardstick's file."""
    import torch
    records, family = S.families()
    rows, exp_off, exp_pairs, exp_scores, exp_labels, n_clusters, n_linked = S.families_expected()
    p = S.FAMILY_PARAMS
    n, text = len(records), family_text(records)
    cap_r = (len(text) + 1) // 2
    d_text = _to(np.frombuffer(text, dtype=np.uint8).copy())
    d_data, d_offs = torch.zeros(len(text), dtype=torch.uint8, device=_dev()), torch.zeros(cap_r + 1, dtype=torch.int64, device=_dev())
    d_spans = torch.zeros((2, cap_r, 2), dtype=torch.int64, device=_dev())
    ctx.fasta_parse_device(d_text, len(text), d_data, len(text), d_offs, cap_r, d_spans[0], d_spans[1])
    assert ctx.fasta_parse_status()[0] == n
    d_rows = torch.zeros(n * 256, dtype=torch.int64, device=_dev())
    cap = n * p["n_bands"]
    d_pair_off, d_pairs = torch.zeros(n + 1, dtype=torch.int64, device=_dev()), torch.zeros(2 * cap, dtype=torch.int32, device=_dev())
    d_scores, d_labels = torch.zeros(2 * cap, dtype=torch.int32, device=_dev()), torch.zeros(n, dtype=torch.int64, device=_dev())
    ctx.sketch_batch_device(d_data, d_offs, n, d_rows, k=p["k"], log2_bins=p["log2_bins"])
    ctx.cluster_candidates_device(d_rows, n, p["log2_bins"], d_pair_off, d_pairs, cap, n_bands=p["n_bands"], band_bins=p["band_bins"])
    total = ctx.cluster_candidates_status()
    ctx.sketch_compare_device(d_rows, n, d_rows, n, p["log2_bins"], d_pairs, total, d_scores)
    ctx.cluster_link_device(n, d_pairs, d_scores, total, d_labels, n_bands=p["n_bands"], band_bins=p["band_bins"], min_similarity=p["min_similarity"],
                            min_filled=p["min_filled"])
    d_kept, d_kept_off = torch.zeros(len(text), dtype=torch.uint8, device=_dev()), torch.zeros(n + 1, dtype=torch.int64, device=_dev())
    d_src, d_dup = torch.zeros(n, dtype=torch.int64, device=_dev()), torch.zeros((2, n), dtype=torch.int64, device=_dev())
    ctx.uniq_compact_device(d_data, d_offs, n, d_labels, d_kept, d_kept_off, d_src, 0, d_dup[0], d_dup[1])
    assert ctx.cluster_link_status() == (n_clusters, n_linked, 0) and ctx.sketch_compare_status() == 0
    m, kept_bytes = ctx.uniq_compact_status()
    d_out, d_out_off = torch.zeros(2 * len(text), dtype=torch.uint8, device=_dev()), torch.zeros(m + 1, dtype=torch.int64, device=_dev())
    ctx.fasta_write_device(d_text, len(text), d_spans[0], n, m, d_out, 2 * len(text), d_out_off, d_body=d_kept, d_body_offsets=d_kept_off, d_src=d_src, n_src=m)
    written, bad = ctx.fasta_write_status()
    assert np.array_equal(d_rows.cpu().numpy().view(np.uint64).reshape(n, 256), rows)
    assert total == len(exp_pairs) and np.array_equal(d_pair_off.cpu().numpy().view(np.uint64), exp_off)
    assert np.array_equal(d_pairs.cpu().numpy().view(np.uint32)[:2 * total].reshape(-1, 2), exp_pairs)
    assert np.array_equal(d_scores.cpu().numpy().view(np.uint32)[:2 * total].reshape(-1, 2), exp_scores)
    labels = d_labels.cpu().numpy().view(np.uint64)
    assert np.array_equal(labels, exp_labels) and np.array_equal(labels, S.family_labels(family)) and m == n_clusters == 120 and bad == 0
    reps = [i for i in range(n) if exp_labels[i] == i]
    assert d_out[:written].cpu().numpy().tobytes() == b"".join(b">rec%d family words\n" % i + records[i] + b"\n" for i in reps)
    dup = d_dup[:, :n - m].cpu().numpy().view(np.uint64)
    members = [i for i in range(n) if exp_labels[i] != i]
    assert dup[0].tolist() == members and dup[1].tolist() == [int(exp_labels[i]) for i in members]


def test_the_host_form_and_the_driver(ctx):
    import circkit_amd
    from circkit_amd import cluster
    records, family = S.families()
    exp_labels, n_clusters = S.families_expected()[4], S.families_expected()[5]
    labels, m = circkit_amd.cluster_batch(records)
    assert labels.dtype == np.uint64 and np.array_equal(labels, exp_labels) and m == n_clusters
    high = S.families_expected(0.9)
    labels9, m9 = circkit_amd.cluster_batch(records, min_similarity=0.9)
    assert np.array_equal(labels9, high[4]) and m9 == high[5] > n_clusters
    fasta, table, driver_labels = cluster.cluster_fasta(family_text(records))
    assert np.array_equal(driver_labels, labels)
    reps = [i for i in range(len(records)) if exp_labels[i] == i]
    assert fasta == b"".join(b">rec%d family words\n" % i + records[i] + b"\n" for i in reps)
    assert table == b"member\trepresentative\n" + b"".join(b"rec%d\trec%d\n" % (i, int(exp_labels[i])) for i in range(len(records)) if exp_labels[i] != i)
    none = circkit_amd.cluster_batch([])
    assert none[1] == 0 and len(none[0]) == 0
    assert cluster.cluster_fasta(b"")[0] == b""
    # refused from the offsets alone, and parameters that do not fit the row
    from circkit_amd import api
    data = np.frombuffer(b"ACGTACGTAC", dtype=np.uint8)
    out, cnt = np.full(2, 7, dtype=np.uint64), ctypes.c_uint64(7)
    sp, p = api.sketch_params(k=4, log2_bins=4), api.cluster_params(n_bands=4, band_bins=2)
    for offs, code in (([0, 10, 10 + 2 ** 31], TOO_LONG), ([1, 10, 10], INVALID_ARG), ([0, 10, 4], INVALID_ARG)):
        offs = np.array(offs, dtype=np.uint64)
        assert ctx._lib.circkit_cluster_batch(ctx._h, api._ptr(data), api._ptr(offs), 2, ctypes.byref(sp), ctypes.byref(p), api._ptr(out), ctypes.byref(cnt)) == code
    offs = np.array([0, 5, 10], dtype=np.uint64)
    wide = api.cluster_params(n_bands=16, band_bins=2)
    assert ctx._lib.circkit_cluster_batch(ctx._h, api._ptr(data), api._ptr(offs), 2, ctypes.byref(sp), ctypes.byref(wide), api._ptr(out), ctypes.byref(cnt)) == INVALID_ARG
    assert (out == 7).all() and cnt.value == 7


def test_the_labels_are_invariant(ctx):
    """Every record rotated, and every record reverse-complemented, through the project's own device calls: the same labels."""
    import circkit_amd
    records, _ = S.families()
    exp_labels = S.families_expected()[4]
    data, offs = SS.pack(records)
    for name, (d2, o2) in (("rotate", ctx.rotate_batch(data, offs, bases=123)), ("rotate %", ctx.rotate_batch(data, offs, percent=0.41)),
                           ("revcomp", ctx.revcomp_batch(data, offs))):
        assert not np.array_equal(d2, data), name
        labels, m = circkit_amd.default_context().cluster_batch(d2, o2)
        assert np.array_equal(labels, exp_labels) and m == 120, name
