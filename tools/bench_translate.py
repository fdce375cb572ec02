#!/usr/bin/env python
"""Throughput of circkit_windows_translate_device on one MI355X: device-resident batches, median of 5 runs after 2 warm-ups, each
figure with its stream wait, one case per process, per case one JSON line:

  orf_seqs   the proteins of the ORF batch of 10M x 1 kb records under the CLI's default flags (min_length 75, a stop required,
             both strands; windows from circkit_orfs_windows_device; the stop codons cut): tools/bench_windows.py's case
  revcomp    one full-length strand-1 window per record of the same batch

  translate  the five kernels of a translate (residue counts, tile sums, scan, apply, translate) + the stream wait; table 1
  gather     circkit_windows_gather_device over the same windows: the same source bytes, three times the stores
  copy       circkit_bench_copy_device (best of its variants) over half of the bytes the translate reads plus writes: a copy
             of B bytes reads B and writes B

    python tools/bench_translate.py --case orf_seqs|revcomp [--records N]
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
    ap.add_argument("--case", default="orf_seqs", choices=("orf_seqs", "revcomp"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_translate: no HIP device")
    import circkit_amd
    from circkit_amd import api, workloads
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.records
    d_bytes, d_offs = workloads.fixed_length(ctx, dev, n, L)
    ctx.synchronize()
    if a.case == "revcomp":
        m = n
        d_win = torch.empty(m * 24, dtype=torch.uint8, device=dev)
        ctx.windows_of_records_device(d_offs, n, "revcomp", d_win)
    else:
        d_orf_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        kw = dict(min_length=75, require_stop=True, strands="both", mode="longest")
        ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, None, 0, **kw)            # the count, for the room
        ctx.synchronize()
        m = int(d_orf_off[n].item())
        d_orfs = torch.empty(m * 24, dtype=torch.uint8, device=dev)
        ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, m, **kw)
        assert ctx.orfs_status() == m
        d_win = torch.empty(m * 24, dtype=torch.uint8, device=dev)
        ctx.orfs_windows_device(d_orf_off, d_orfs, n, m, d_win)
        ctx.synchronize()
        del d_orfs, d_orf_off
    d_out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
    ctx.windows_gather_device(d_bytes, d_offs, n, d_win, m, None, 0, d_out_off)        # the totals, for the room
    ctx.synchronize()
    seq_bytes = int(d_out_off[m].item())
    params = api.translate_params(table=1)
    ctx.windows_translate_device(d_bytes, d_offs, n, d_win, m, None, 0, d_out_off, params=params)
    ctx.synchronize()
    residues = int(d_out_off[m].item())
    d_out = torch.empty(seq_bytes + 64, dtype=torch.uint8, device=dev)
    t_translate = timed(ctx, lambda: ctx.windows_translate_device(d_bytes, d_offs, n, d_win, m, d_out, residues, d_out_off, params=params),
                        a.steps, a.warmup)
    assert ctx.translate_status() == (residues, 0)
    t_gather = timed(ctx, lambda: ctx.windows_gather_device(d_bytes, d_offs, n, d_win, m, d_out, seq_bytes, d_out_off), a.steps, a.warmup)
    assert ctx.windows_status() == (seq_bytes, 0)
    read = 3 * residues                                      # the symbols the residues are made of
    half = (read + residues) // 2 // 16 * 16
    assert half <= d_bytes.numel() and half <= d_out.numel()
    copies = {v: timed(ctx, lambda: ctx.bench_copy_device(d_bytes, d_out, half, v), a.steps, a.warmup) for v in range(5)}
    v = min(copies, key=copies.get)
    moved = read + residues + m * (2 * 24 + 5 * 8)           # + per window: its 24 bytes read twice, the 8 of its offset written twice, read three times
    print(json.dumps({
        "case": a.case, "records": n, "windows": m, "bytes_read": read, "bytes_written": residues, "translate_seconds": round(t_translate, 6),
        "translate_bytes_moved": moved, "translate_bytes_per_s": round(moved / t_translate), "gather_bytes_written": seq_bytes,
        "gather_seconds": round(t_gather, 6), "copy_bytes": half, "copy_seconds": round(copies[v], 6), "copy_variant": v,
        "copy_bytes_per_s": round(2 * half / copies[v]), "translate_over_gather": round(t_translate / t_gather, 3),
        "translate_over_copy": round(t_translate / copies[v], 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
