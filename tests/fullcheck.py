"""Whole-batch oracle check for batches too large to copy to the host at once (the full-size GPU tests).

check_batch() walks a CSR batch in record-aligned chunks of about `chunk_bytes` of payload: each chunk of the input and of
every output given is copied to the host, its offsets are rebased to 0, the CPU oracle (oracle/circkit_oracle.c) runs on
it with one thread per CPU this process may use, and the outputs are compared record by record.  First-seen indices are
compared against the oracle's first-seen map over the hashes of the WHOLE batch, so a duplicate in an earlier chunk counts.
Host memory stays at a few chunks (plus 8 bytes per record for the offsets and, with first_seen, the hashes): the 10 GB
batches are never copied whole.  Works on CUDA tensors, CPU tensors and numpy arrays alike.
"""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def _host(t, a, b, dtype):
    """t[a:b] as a host numpy array of `dtype` (same item size: a reinterpretation, e.g. int64 -> uint64)."""
    v = t[a:b]
    if hasattr(v, "cpu"):
        v = v.cpu().numpy()
    return np.ascontiguousarray(v).view(dtype)


def synth_input(O, seed, first_base, threads=None):
    """host_input for check_batch: bytes [b0, b1) of the batch are bases first_base + b0 .. of the counter-based generator
    (O.synth_fill), generated on `threads` threads."""
    threads = threads or len(os.sched_getaffinity(0))

    def fill(b0, b1):
        n = b1 - b0
        cuts = [b0 + n * k // threads for k in range(threads + 1)]
        with ThreadPoolExecutor(threads) as ex:
            parts = list(ex.map(lambda k: O.synth_fill(seed, first_base + cuts[k], cuts[k + 1] - cuts[k]), range(threads)))
        return np.concatenate(parts) if parts else np.empty(0, np.uint8)
    return fill


def _where(off, r, what):
    o = int(off[r])
    return "%s differs at record %d (length %d, byte offset %d = 0x%x, %s 2^32)" % (
        what, r, int(off[r + 1]) - o, o, o, ">=" if o >= 1 << 32 else "<")


def check_batch(O, d_bytes, d_offsets, n, *, out_bytes=None, out_xxh3=None, out_index=None, out_strand=None, first_seen=None,
                chunk_bytes=256 << 20, host_input=None):
    """Asserts that every record of the batch (d_bytes, d_offsets[0..n]) has the oracle's canonical bytes (out_bytes: uint8,
    same layout as the input), XXH3 (out_xxh3: 64-bit), rotation index (out_index: 32-bit), strand (out_strand: uint8) and
    first-seen index (first_seen: 64-bit, relative to record 0 of this batch); every output is optional.
    host_input(b0, b1) -> uint8 array, optional: the input bytes [b0, b1) made on the host -- they must equal d_bytes there and
    are what the oracle runs on.  Returns what was compared: records, the last record's index and byte offset, seconds."""
    t0 = time.time()
    threads = len(os.sched_getaffinity(0))
    off = _host(d_offsets, 0, n + 1, np.uint64)
    want_hash = out_xxh3 is not None or first_seen is not None
    all_h = np.empty(n, np.uint64) if first_seen is not None else None

    chunks = []
    r0 = 0
    while r0 < n:
        r1 = int(np.searchsorted(off, off[r0] + np.uint64(chunk_bytes), side="right")) - 1
        r1 = min(n, max(r1, r0 + 1))
        chunks.append((r0, r1))
        r0 = r1

    def fetch(c):
        r0, r1 = c
        b0, b1 = int(off[r0]), int(off[r1])
        h = {"in": _host(d_bytes, b0, b1, np.uint8)}
        if host_input is not None:
            made = np.asarray(host_input(b0, b1), dtype=np.uint8)
            if not np.array_equal(made, h["in"]):
                p = int(np.flatnonzero(made != h["in"])[0])
                r = r0 + int(np.searchsorted(off[r0:r1 + 1], np.uint64(b0 + p), side="right")) - 1
                raise AssertionError(_where(off, r, "input (device bytes vs the host generator)") +
                                     ": byte %d of the record, device 0x%02x, host 0x%02x" % (b0 + p - int(off[r]), h["in"][p], made[p]))
            h["in"] = made
        if out_bytes is not None:
            h["bytes"] = _host(out_bytes, b0, b1, np.uint8)
        for k, t, dt in (("xxh3", out_xxh3, np.uint64), ("index", out_index, np.uint32), ("strand", out_strand, np.uint8)):
            if t is not None:
                h[k] = _host(t, r0, r1, dt)
        return h

    with ThreadPoolExecutor(1) as ex:              # the next chunk is copied while the oracle runs on this one
        nxt = ex.submit(fetch, chunks[0]) if chunks else None
        for k, (r0, r1) in enumerate(chunks):
            h = nxt.result()
            nxt = ex.submit(fetch, chunks[k + 1]) if k + 1 < len(chunks) else None
            loc = off[r0:r1 + 1] - off[r0]
            exp, exp_h, exp_i, exp_s = O.canonicalize_batch_aux(h["in"], loc, out_bytes is not None, want_hash, out_index is not None,
                                                               out_strand is not None, threads=threads)
            if out_bytes is not None and not np.array_equal(h["bytes"], exp):
                p = int(np.flatnonzero(h["bytes"] != exp)[0])
                r = r0 + int(np.searchsorted(loc, np.uint64(p), side="right")) - 1
                q = p - int(loc[r - r0])
                raise AssertionError(_where(off, r, "canonical bytes") + ": first at byte %d of the record, got 0x%02x, expected 0x%02x"
                                     % (q, h["bytes"][p], exp[p]))
            for name, e in (("xxh3", exp_h), ("index", exp_i), ("strand", exp_s)):
                if name in h and not np.array_equal(h[name], e):
                    i = int(np.flatnonzero(h[name] != e)[0])
                    raise AssertionError(_where(off, r0 + i, name) + ": got %d, expected %d" % (int(h[name][i]), int(e[i])))
            if all_h is not None:
                all_h[r0:r1] = exp_h
    if first_seen is not None:
        exp_fs = O.uniq_first_seen(all_h)
        got_fs = _host(first_seen, 0, n, np.uint64)
        if not np.array_equal(got_fs, exp_fs):
            i = int(np.flatnonzero(got_fs != exp_fs)[0])
            raise AssertionError(_where(off, i, "first_seen") + ": got %d, expected %d" % (int(got_fs[i]), int(exp_fs[i])))
    last = max(n - 1, 0)
    return {"records": n, "last_record": last, "last_record_offset": int(off[last]) if n else 0, "end_offset": int(off[n]),
            "chunks": len(chunks), "threads": threads, "seconds": round(time.time() - t0, 2)}
