"""A plain restatement of the writer closure of `circkit monomerize` (src/monomerize.rs:90-131) for a CSR batch (TEST
INFRASTRUCTURE ONLY): the five rules of the compact and the packing, in numpy.  The GPU compact and its CPU fiber build are
checked against this; tests/test_monomers_compact_cpu.py checks this against tests/mono_ref.py's writer, which is pinned to
the reference's fixtures."""
import numpy as np

NONE = 0xFFFFFFFF
FILTER_KEYS = ("min_length", "max_length", "min_overlap", "min_overlap_percent", "keep_all")


def decide(lengths, ends, full_len=None, min_length=0, max_length=None, min_overlap=None, min_overlap_percent=None, keep_all=False):
    """(kept_end uint32[n], written bool[n], written_length uint64[n]) for records of `lengths` normalized symbols."""
    n = np.asarray(lengths, dtype=np.uint64)
    e = np.asarray(ends, dtype=np.uint32)
    f = n if full_len is None else np.asarray(full_len, dtype=np.uint64)
    idx = e.astype(np.uint64)
    some = (e != NONE) & (idx <= n)                                                        # 1: None, or an end beyond the record
    some &= ~((idx < np.uint64(min_length)) | (idx > np.uint64(2 ** 64 - 1 if max_length is None else max_length)))       # 2
    over = np.where(f > idx, f - idx, np.uint64(0)).astype(np.uint64)                      # saturating: callers owe f >= n
    if min_overlap is not None:
        some &= ~(over < np.uint64(min_overlap))                                           # 3
    if min_overlap_percent is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = over.astype(np.float64) / idx.astype(np.float64)                       # 4: one f64 division; x / 0 is inf or NaN
            some &= ~(ratio < np.float64(min_overlap_percent))                             # a NaN on either side never rejects
    kept = np.where(some, e, np.uint32(NONE)).astype(np.uint32)                            # 5
    written = some | bool(keep_all)
    return kept, written, np.where(some, idx, n).astype(np.uint64)


def compact(data, offsets, ends, full_len=None, **filter):
    """(out_data, out_offsets, out_src, kept_end) of the batch: the written records' first written_length bytes back to back."""
    data = np.asarray(data, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64)
    kept, written, wlen = decide(offsets[1:] - offsets[:-1], ends, full_len, **filter)
    out_src = np.nonzero(written)[0].astype(np.uint64)
    lens = wlen[written].astype(np.int64)
    out_offsets = np.zeros(len(out_src) + 1, dtype=np.uint64)
    out_offsets[1:] = np.cumsum(lens)
    total = int(out_offsets[-1])
    # output byte x of record j comes from offsets[out_src[j]] + (x - out_offsets[j])
    rec = np.repeat(np.arange(len(out_src), dtype=np.int64), lens)
    src = offsets[out_src].astype(np.int64)[rec] + (np.arange(total, dtype=np.int64) - out_offsets[:-1].astype(np.int64)[rec])
    return data[src], out_offsets, out_src, kept


def compact_slow(data, offsets, ends, full_len=None, min_length=0, max_length=None, min_overlap=None, min_overlap_percent=None,
                 keep_all=False):
    """The same, record by record in plain Python, as the issue states the rules (the vectorized form is checked against it)."""
    out, out_offsets, out_src, kept = [], [0], [], []
    for i in range(len(offsets) - 1):
        o, n = int(offsets[i]), int(offsets[i + 1]) - int(offsets[i])
        f = n if full_len is None else int(full_len[i])
        e = int(ends[i])
        idx = None if e == NONE or e > n else e
        if idx is not None and (idx < min_length or (max_length is not None and idx > max_length)):
            idx = None
        if idx is not None and min_overlap is not None and max(f - idx, 0) < min_overlap:
            idx = None
        if idx is not None and min_overlap_percent is not None:
            over = float(max(f - idx, 0))
            ratio = over / float(idx) if idx else (float("inf") if over else float("nan"))
            if ratio < min_overlap_percent:
                idx = None
        kept.append(NONE if idx is None else idx)
        if idx is not None or keep_all:
            w = n if idx is None else idx
            out.append(bytes(data[o:o + w]))
            out_offsets.append(out_offsets[-1] + w)
            out_src.append(i)
    return (np.frombuffer(b"".join(out), dtype=np.uint8), np.array(out_offsets, dtype=np.uint64), np.array(out_src, dtype=np.uint64),
            np.array(kept, dtype=np.uint32))


def assert_equal(got, exp, what=""):
    for name, g, x in zip(("out_data", "out_offsets", "out_src", "kept_end"), got, exp):
        g, x = np.asarray(g), np.asarray(x)
        assert g.shape == x.shape, (what, name, g.shape, x.shape)
        bad = np.nonzero(g != x)[0]
        assert len(bad) == 0, (what, name, int(bad[0]), int(g[bad[0]]), int(x[bad[0]]), len(bad))
