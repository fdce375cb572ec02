"""A plain restatement of the writer side of `circkit uniq` (src/uniq.rs:47-66) for a CSR batch (TEST INFRASTRUCTURE ONLY):
the keep mask, the kept records' slices, out_src and the dropped list, in numpy.  The GPU compact is checked against this;
tests/test_uniq_compact_cpu.py checks this against oracle.cli_uniq, which is pinned to the reference's fixtures."""
import numpy as np

NOT_FOUND = 2 ** 64 - 1
NAMES = ("out_data", "out_offsets", "out_src", "dup_src", "dup_first")


def keep_mask(first_seen, base_index=0):
    """Record i is kept iff first_seen[i] == base_index + i; any other value drops it, ~0 included."""
    fs = np.asarray(first_seen, dtype=np.uint64)
    return fs == np.uint64(base_index) + np.arange(len(fs), dtype=np.uint64)


def compact(data, offsets, first_seen, base_index=0):
    """(out_data, out_offsets, out_src, dup_src, dup_first): the kept records back to back, the input index of each, and for the
    dropped records, in input order, their input index and their first_seen (a global index)."""
    data = np.asarray(data, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.uint64)
    fs = np.asarray(first_seen, dtype=np.uint64)
    keep = keep_mask(fs, base_index)
    out_src = np.nonzero(keep)[0].astype(np.uint64)
    lens = (offsets[1:] - offsets[:-1])[keep].astype(np.int64)
    out_offsets = np.zeros(len(out_src) + 1, dtype=np.uint64)
    out_offsets[1:] = np.cumsum(lens)
    total = int(out_offsets[-1])
    # output byte x of record j comes from offsets[out_src[j]] + (x - out_offsets[j])
    rec = np.repeat(np.arange(len(out_src), dtype=np.int64), lens)
    src = offsets[out_src].astype(np.int64)[rec] + (np.arange(total, dtype=np.int64) - out_offsets[:-1].astype(np.int64)[rec])
    dup_src = np.nonzero(~keep)[0].astype(np.uint64)
    return data[src], out_offsets, out_src, dup_src, fs[~keep]


def compact_slow(data, offsets, first_seen, base_index=0):
    """The same, record by record in plain Python (the vectorized form is checked against it)."""
    out, out_offsets, out_src, dup_src, dup_first = [], [0], [], [], []
    for i in range(len(offsets) - 1):
        if int(first_seen[i]) == (base_index + i) % 2 ** 64:
            out.append(bytes(data[int(offsets[i]):int(offsets[i + 1])]))
            out_offsets.append(out_offsets[-1] + len(out[-1]))
            out_src.append(i)
        else:
            dup_src.append(i)
            dup_first.append(int(first_seen[i]))
    u64 = lambda a: np.array(a, dtype=np.uint64)
    return np.frombuffer(b"".join(out), dtype=np.uint8), u64(out_offsets), u64(out_src), u64(dup_src), u64(dup_first)


def assert_equal(got, exp, what=""):
    for name, g, x in zip(NAMES, got, exp):
        if g is None:                       # an output that was not asked for
            continue
        g, x = np.asarray(g), np.asarray(x)
        assert g.shape == x.shape, (what, name, g.shape, x.shape)
        bad = np.nonzero(g != x)[0]
        assert len(bad) == 0, (what, name, int(bad[0]), int(g[bad[0]]), int(x[bad[0]]), len(bad))
