#!/usr/bin/env python
"""Throughput of the sketch unit on one MI355X: device-resident batches, stream events, median of 5 runs after 2 warm-ups with the
minimum and maximum; one JSON line.

  fixed      --records x 1 kb random ACGT records, k = 21, at 64 and at 256 bins.  One loop, alternating: circkit_sketch_batch_device
             + circkit_sketch_status, circkit_xxh3_batch_device over the same batch, and circkit_bench_copy_device (the best of its
             variants) over half of the bytes the sketch reads plus writes (a copy of B bytes reads B and writes B)
  mixed      --mixed-records records of 200 b .. 20 kb (P(L) ~ 1/L), 256 bins
  long       one record of 50 M symbols, 256 bins: the span route alone
  compare    --pairs random pairs over the rows of `fixed` at 256 bins, against what a copy at the measured rate would take over the
             2 * bins * 8 bytes a pair reads
  host       circkit_sketch_batch from page-locked host buffers over the first --host-records records of `fixed`, against a
             one-thread C restatement of the definition (tools/sketch_host_ref.c, compiled here) over the same records.  The
             acceptance condition: the host form is not slower; overlapping [min, max] ranges count as equal.  The rows of the
             device form, the host form and the restatement are compared with each other.

    python tools/bench_sketch.py [--records N] [--mixed-records N] [--pairs N] [--host-records N]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, K = 1000, 21


def stats(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 4), "min_ms": round(min(times) * 1e3, 4), "max_ms": round(max(times) * 1e3, 4)}


def event_loop(torch, fns, steps, warmup):
    """Every fn once per round, in turn; per fn the seconds between two events of the stream round its work."""
    times = {name: [] for name in fns}
    for it in range(warmup + steps):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            after = fn()
            t1.record()
            if after:
                after()
            t1.synchronize()
            if it >= warmup:
                times[name].append(t0.elapsed_time(t1) * 1e-3)
    return times


def wall_loop(fn, steps, warmup):
    times = []
    for it in range(warmup + steps):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            times.append(time.perf_counter() - t0)
    return times


def build_host_ref(tmp):
    so = os.path.join(tmp, "libsketch_host_ref.so")
    subprocess.check_call(["cc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "sketch_host_ref.c")])
    lib = ctypes.CDLL(so)
    lib.sketch_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                                ctypes.c_void_p]
    lib.sketch_host.restype = None
    return lib


def pinned(lib, dtype, count):
    """A page-locked numpy array (circkit_host_alloc); the caller frees the address it returns with it."""
    nbytes = max(count * np.dtype(dtype).itemsize, 1)
    p = lib.circkit_host_alloc(nbytes)
    if not p:
        sys.exit("bench_sketch: circkit_host_alloc failed")
    return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p), dtype=dtype, count=count), p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--mixed-records", type=int, default=200_000)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    ap.add_argument("--host-records", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_sketch: no HIP device")
    import circkit_amd
    from circkit_amd import api, workloads
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"k": K, "records": a.records, "record_length": L}

    # ---- fixed: 64 and 256 bins, the hash pass and the copy in the same loop ------------------------------------------------
    n = a.records
    d_bytes, d_offs = workloads.fixed_length(ctx, dev, n, L)
    d_rows = torch.empty(n * 256 + 2, dtype=torch.int64, device=dev)
    d_counts = torch.empty(n, dtype=torch.int32, device=dev)
    d_hash = torch.empty(n, dtype=torch.int64, device=dev)
    ctx.synchronize()
    copy_rate = None
    for log2_bins in (6, 8):
        moved = n * L + (n + 1) * 8 + n * (8 << log2_bins) + n * 4
        half = moved // 2 // 16 * 16
        half = min(half, d_bytes.numel() // 16 * 16)                  # (the copy's rate is what is used: it reads d_bytes and writes over d_rows)
        copies = {v: statistics.median(event_loop(torch, {"c": lambda v=v: ctx.bench_copy_device(d_bytes, d_rows, half, v)}, 3, 1)["c"]) for v in range(5)}
        best = min(copies, key=copies.get)
        p = api.sketch_params(k=K, log2_bins=log2_bins)
        t = event_loop(torch, {
            "sketch": lambda: (ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows, d_counts, params=p), ctx.sketch_status)[1],
            "xxh3": lambda: ctx.xxh3_batch_device(d_bytes, d_offs, n, d_hash),
            "copy": lambda: ctx.bench_copy_device(d_bytes, d_rows, half, best)}, a.steps, a.warmup)
        assert ctx.sketch_status() == (n * L, 0)
        med = {name: statistics.median(v) for name, v in t.items()}
        copy_rate = 2 * half / med["copy"]
        out["bins%d" % (1 << log2_bins)] = {
            "sketch": stats(t["sketch"]), "xxh3": stats(t["xxh3"]), "copy": stats(t["copy"]), "copy_variant": best, "copy_bytes": half,
            "sketch_bytes_moved": moved, "copy_bytes_per_s": round(copy_rate), "kmers_per_s": round(n * L / med["sketch"]),
            "copy_time_for_sketch_bytes_ms": round(moved / copy_rate * 1e3, 4), "fraction_of_copy": round(moved / copy_rate / med["sketch"], 4),
            "sketch_over_xxh3": round(med["sketch"] / med["xxh3"], 3)}
    ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows, d_counts, params=p)      # the copy wrote over the rows: the 256-bin rows once more
    assert ctx.sketch_status() == (n * L, 0)

    # ---- compare over random pairs ------------------------------------------------------------------------------------------
    m = a.pairs
    d_pairs = torch.randint(0, n, (m, 2), dtype=torch.int32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    d_res = torch.empty((m, 2), dtype=torch.int32, device=dev)
    t = event_loop(torch, {"compare": lambda: (ctx.sketch_compare_device(d_rows, n, d_rows, n, 8, d_pairs, m, d_res), ctx.sketch_compare_status)[1]},
                   a.steps, a.warmup)["compare"]
    read = m * (2 * 256 * 8 + 8) + m * 8
    out["compare"] = {"pairs": m, "bins": 256, **stats(t), "bytes_moved": read, "pairs_per_s": round(m / statistics.median(t)),
                      "copy_time_for_bytes_ms": round(read / copy_rate * 1e3, 4), "fraction_of_copy": round(read / copy_rate / statistics.median(t), 4)}
    del d_pairs, d_res

    # ---- host: page-locked buffers against the one-thread restatement ---------------------------------------------------------
    nh = min(a.host_records, n)
    lib = ctx._lib
    h_bytes, p0 = pinned(lib, np.uint8, nh * L)
    h_offs, p1 = pinned(lib, np.uint64, nh + 1)
    h_rows, p2 = pinned(lib, np.uint64, nh * 256)
    h_counts, p3 = pinned(lib, np.uint32, nh)
    h_bytes[:] = d_bytes[:nh * L].cpu().numpy()
    h_offs[:] = np.arange(nh + 1, dtype=np.uint64) * L
    p = api.sketch_params(k=K, log2_bins=8)

    def host_form():
        rc = lib.circkit_sketch_batch(ctx._h, h_bytes.ctypes.data, h_offs.ctypes.data, nh, ctypes.byref(p), h_rows.ctypes.data, h_counts.ctypes.data)
        assert rc == 0, rc

    t_host = wall_loop(host_form, a.steps, a.warmup)
    with tempfile.TemporaryDirectory() as tmp:
        ref = build_host_ref(tmp)
        c_rows, c_counts = np.empty(nh * 256, dtype=np.uint64), np.empty(nh, dtype=np.uint32)
        t_ref = wall_loop(lambda: ref.sketch_host(h_bytes.ctypes.data, h_offs.ctypes.data, nh, K, 8, 0, c_rows.ctypes.data, c_counts.ctypes.data),
                          max(a.steps - 2, 1), 1)
    dev_rows = d_rows[:nh * 256].cpu().numpy().view(np.uint64)
    rows_agree = bool(np.array_equal(h_rows, c_rows) and np.array_equal(h_rows, dev_rows) and np.array_equal(h_counts, c_counts))
    out["host"] = {"records": nh, "host_form": stats(t_host), "one_thread_c": stats(t_ref), "rows_agree": rows_agree,
                   "host_form_not_slower": bool(min(t_host) <= max(t_ref))}
    for q in (p0, p1, p2, p3):
        lib.circkit_host_free(q)
    del d_bytes, d_offs, d_rows, d_counts, d_hash

    # ---- mixed lengths and one long record --------------------------------------------------------------------------------------
    offs = workloads.log_uniform_offsets(a.mixed_records)
    total = int(offs[-1])
    d_offs = offs.to(dev)
    d_bytes = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    ctx.synth_fill_device(45, 0, total, d_bytes)
    d_rows = torch.empty(a.mixed_records * 256, dtype=torch.int64, device=dev)
    p = api.sketch_params(k=K, log2_bins=8)
    t = event_loop(torch, {"s": lambda: (ctx.sketch_batch_device(d_bytes, d_offs, a.mixed_records, d_rows, None, params=p), ctx.sketch_status)[1]},
                   a.steps, a.warmup)["s"]
    lens = (offs[1:] - offs[:-1])
    assert ctx.sketch_status() == (int(lens[lens >= K].sum()), 0)
    out["mixed"] = {"records": a.mixed_records, "symbols": total, "long_records": int((lens > 4096).sum()), **stats(t),
                    "kmers_per_s": round(total / statistics.median(t))}
    del d_bytes, d_offs, d_rows
    big = 50_000_000
    d_bytes = torch.empty(big + 64, dtype=torch.uint8, device=dev)
    ctx.synth_fill_device(46, 0, big, d_bytes)
    d_offs = torch.tensor([0, big], dtype=torch.int64, device=dev)
    d_rows = torch.empty(256, dtype=torch.int64, device=dev)
    t = event_loop(torch, {"s": lambda: (ctx.sketch_batch_device(d_bytes, d_offs, 1, d_rows, None, params=p), ctx.sketch_status)[1]}, a.steps, a.warmup)["s"]
    assert ctx.sketch_status() == (big, 0)
    out["long"] = {"symbols": big, **stats(t), "kmers_per_s": round(big / statistics.median(t))}
    print(json.dumps(out), flush=True)
    ctx.close()
    if not (rows_agree and out["host"]["host_form_not_slower"]):
        sys.exit("bench_sketch: the acceptance condition does not hold")


if __name__ == "__main__":
    main()
