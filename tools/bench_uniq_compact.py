#!/usr/bin/env python
"""Throughput of circkit_uniq_compact_device on one MI355X, and of the chain it closes: 10M x 1 kb device-resident records,
duplicate fractions 0, 0.5 and 0.9, median of 5 runs after 2 warm-ups, one process, per fraction one JSON line:

  compact   circkit_uniq_compact_device (decide, scan, apply with the dropped list, gather) + the stream wait, of the canonical
            bytes, on a first_seen computed once
  nothing   the same on a first_seen that keeps no record: decide, scan, apply and the launches without a byte packed
  chain     canonicalize_batch_device (bytes + xxh3) -> uniq_resolve_device -> the compact + the wait
  copy      circkit_bench_copy_device (best of its variants) over the kept bytes: the yardstick.  The compact reads and writes
            each kept byte once, plus 8 bytes of first_seen and up to 24 bytes of indices per record

Record i of the batch is a copy of record i mod k, k = the number of distinct records; the records are uniform ACGT.

    python tools/bench_uniq_compact.py [--records N] [--fractions 0,0.5,0.9]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = 1000


def timed(ctx, fn, steps, warmup):
    times = []
    for it in range(warmup + steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        if it >= warmup:
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--fractions", default="0,0.5,0.9")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_uniq_compact: no HIP device")
    import circkit_amd
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n, nb = a.records, a.records * L
    d_bytes = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    d_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_canon = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    d_out = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
    d_hash, d_fs, d_none, d_out_src, d_dup_src, d_dup_first = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(6))
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_none.fill_(-1)                                       # ~0: no record is kept
    ctx.fixed_offsets_device(0, L, n, d_offs)
    for frac in (float(x) for x in a.fractions.split(",")):
        k = max(1, int(round(n * (1.0 - frac))))
        ctx.synth_fill_device(2027, 0, k * L, d_bytes)
        ctx.synchronize()
        rows = d_bytes[:nb].view(n, L)
        for lo in range(k, n, 1 << 20):                    # record i = record i mod k, a slab at a time
            hi = min(lo + (1 << 20), n)
            rows[lo:hi] = rows[torch.arange(lo, hi, device=dev) % k]
        torch.cuda.synchronize()

        def canonicalize():
            ctx.canonicalize_batch_device(d_bytes, d_offs, n, out_bytes=d_canon, out_xxh3=d_hash)

        def resolve():
            ctx.uniq_resolve_device(d_hash, n, 0, d_fs)

        def compact(fs=d_fs):
            ctx.uniq_compact_device(d_canon, d_offs, n, fs, d_out, d_out_off, d_out_src, d_dup_src=d_dup_src, d_dup_first=d_dup_first)

        def chain():
            canonicalize()
            resolve()
            compact()

        t_canon = timed(ctx, canonicalize, a.steps, a.warmup)
        t_resolve = timed(ctx, resolve, a.steps, a.warmup)
        ctx.uniq_status()
        t_nothing = timed(ctx, lambda: compact(d_none), a.steps, a.warmup)
        assert ctx.uniq_compact_status() == (0, 0)
        t_compact = timed(ctx, compact, a.steps, a.warmup)
        m, B = ctx.uniq_compact_status()
        t_chain = timed(ctx, chain, a.steps, a.warmup)
        assert ctx.uniq_compact_status() == (m, B)
        copies = {}
        b16 = B // 16 * 16
        for v in range(5):
            copies[v] = timed(ctx, lambda: ctx.bench_copy_device(d_canon, d_out, b16, v), a.steps, a.warmup) if b16 else 0.0
        best = min(copies, key=copies.get)
        t_copy = copies[best]
        moved = 2 * B + n * 8 + m * 16 + (n - m) * 16 + n * 8          # kept bytes in and out, first_seen, index outputs, the offsets read
        print(json.dumps({
            "records": n, "record_bytes": L, "duplicate_fraction": frac, "distinct_records": k, "kept_records": m, "kept_bytes": B,
            "compact_seconds": round(t_compact, 6), "compact_nothing_kept_seconds": round(t_nothing, 6),
            "compact_bytes_moved": moved, "compact_bytes_per_s": round(moved / t_compact),
            "copy_seconds": round(t_copy, 6), "copy_variant": best, "copy_bytes_per_s": round(2 * b16 / t_copy) if t_copy else None,
            "compact_over_copy": round(t_compact / t_copy, 3) if t_copy else None,
            "canonicalize_xxh3_seconds": round(t_canon, 6), "uniq_resolve_seconds": round(t_resolve, 6),
            "sum_of_parts_seconds": round(t_canon + t_resolve + t_compact, 6), "chain_seconds": round(t_chain, 6)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
