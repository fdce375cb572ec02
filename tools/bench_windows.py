#!/usr/bin/env python
"""Throughput of circkit_windows_gather_device on one MI355X: device-resident batches, median of 5 runs after 2 warm-ups, one
process, per case one JSON line:

  rotate     every record of 10M x 1 kb rotated by 0.37 of its length (windows from circkit_windows_of_records_device)
  revcomp    the reverse complement of the same records
  cat        every record of 5M x 1 kb twice in a row
  orf_seqs   the sequences of the ORF batch of the 10M x 1 kb records under the CLI's default flags (min_length 75, a stop
             required, both strands; windows from circkit_orfs_windows_device; the stop codons cut)
  rotate_mixed  rotate by 0.37 on the mixed-length batch (P(L) ~ 1/L on [200, 20000], circkit_amd.workloads), as many bytes

  gather     the five kernels of a gather (lengths, tile sums, scan, apply, gather) + the stream wait
  windows    the kernel that writes the windows, + the wait (not part of `gather`)
  copy       circkit_bench_copy_device (best of its variants) over as many bytes as the gather reads plus writes, halved: a copy
             of B bytes reads B and writes B.  The gather also moves 88 bytes per window (its 24 bytes read twice, the 8 of its
             offset written twice and read three times); `gather_bytes_moved` counts them, `copy` does not move them.

    python tools/bench_windows.py [--records N] [--cases rotate,revcomp,cat,orf_seqs,rotate_mixed]
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
    ap.add_argument("--cases", default="rotate,revcomp,cat,orf_seqs,rotate_mixed")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_windows: no HIP device")
    import circkit_amd
    from circkit_amd import workloads
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.records
    d_bytes, d_offs = workloads.fixed_length(ctx, dev, n, L)
    ctx.synchronize()

    def best_copy(d_src, d_dst, nbytes):
        b16 = nbytes // 16 * 16
        copies = {v: timed(ctx, lambda: ctx.bench_copy_device(d_src, d_dst, b16, v), a.steps, a.warmup) for v in range(5)}
        v = min(copies, key=copies.get)
        return copies[v], v, b16

    def report(case, n_records, n_windows, read_bytes, t_windows, gather, d_payload, d_out):
        t_gather = timed(ctx, gather, a.steps, a.warmup)
        total, bad = ctx.windows_status()
        assert bad == 0
        half = (read_bytes + total) // 2                     # a copy of `half` bytes reads and writes what the gather reads plus writes
        assert half <= d_payload.numel() and half <= d_out.numel()
        t_copy, variant, b16 = best_copy(d_payload, d_out, half)
        moved = read_bytes + total + n_windows * (2 * 24 + 5 * 8)
        print(json.dumps({
            "case": case, "records": n_records, "windows": n_windows, "bytes_read": read_bytes, "bytes_written": total,
            "windows_seconds": round(t_windows, 6), "gather_seconds": round(t_gather, 6), "gather_bytes_moved": moved,
            "gather_bytes_per_s": round(moved / t_gather), "copy_bytes": b16, "copy_seconds": round(t_copy, 6), "copy_variant": variant,
            "copy_bytes_per_s": round(2 * b16 / t_copy), "gather_over_copy": round(t_gather / t_copy, 3)}), flush=True)

    def per_record(case, kind, d_payload, d_off, n_records, nb, out_bytes, **kw):
        d_win = torch.empty(n_records * 24, dtype=torch.uint8, device=dev)
        d_out = torch.empty(max(out_bytes, nb) + 64, dtype=torch.uint8, device=dev)
        d_out_off = torch.empty(n_records + 1, dtype=torch.int64, device=dev)
        t_windows = timed(ctx, lambda: ctx.windows_of_records_device(d_off, n_records, kind, d_win, **kw), a.steps, a.warmup)
        report(case, n_records, n_records, out_bytes if kind != "cat" else nb, t_windows,
               lambda: ctx.windows_gather_device(d_payload, d_off, n_records, d_win, n_records, d_out, out_bytes, d_out_off), d_payload, d_out)

    for case in a.cases.split(","):
        if case == "rotate":
            per_record(case, "rotate_percent", d_bytes, d_offs, n, n * L, n * L, percent=0.37)
        elif case == "revcomp":
            per_record(case, "revcomp", d_bytes, d_offs, n, n * L, n * L)
        elif case == "cat":
            per_record(case, "cat", d_bytes, d_offs, n // 2, (n // 2) * L, 2 * (n // 2) * L)
        elif case == "orf_seqs":
            d_orf_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
            kw = dict(min_length=75, require_stop=True, strands="both", mode="longest")
            ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, None, 0, **kw)            # the count, for the room
            ctx.synchronize()
            n_orfs = int(d_orf_off[n].item())
            d_orfs = torch.empty(n_orfs * 24, dtype=torch.uint8, device=dev)
            ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, n_orfs, **kw)
            assert ctx.orfs_status() == n_orfs
            d_win = torch.empty(n_orfs * 24, dtype=torch.uint8, device=dev)
            d_seq_off = torch.empty(n_orfs + 1, dtype=torch.int64, device=dev)
            t_windows = timed(ctx, lambda: ctx.orfs_windows_device(d_orf_off, d_orfs, n, n_orfs, d_win), a.steps, a.warmup)
            del d_orfs
            ctx.windows_gather_device(d_bytes, d_offs, n, d_win, n_orfs, None, 0, d_seq_off)      # the total, for the room
            ctx.synchronize()
            total = int(d_seq_off[n_orfs].item())
            d_seq = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            d_src = torch.empty(total + 64, dtype=torch.uint8, device=dev)                       # the copy's source: as many bytes as the sequences
            report(case, n, n_orfs, total, t_windows,
                   lambda: ctx.windows_gather_device(d_bytes, d_offs, n, d_win, n_orfs, d_seq, total, d_seq_off), d_src, d_seq)
            del d_win, d_seq, d_src, d_seq_off, d_orf_off
        elif case == "rotate_mixed":
            offs = workloads.log_uniform_offsets(max(1, n * L // 4300))        # (the mean of 1/L on [200, 20000] is ~ 4 300 symbols)
            nm, nb = len(offs) - 1, int(offs[-1])
            d_moffs = offs.to(dev)
            d_mixed = d_bytes if nb <= n * L else torch.empty(nb + 64, dtype=torch.uint8, device=dev)
            if d_mixed is not d_bytes:
                ctx.synth_fill_device(45, 0, nb, d_mixed)
            per_record(case, "rotate_percent", d_mixed, d_moffs, nm, nb, nb, percent=0.37)
        else:
            sys.exit("bench_windows: unknown case %r" % case)
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
