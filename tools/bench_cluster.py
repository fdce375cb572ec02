#!/usr/bin/env python
"""Time of the cluster unit's steps on one MI355X: a device-resident batch, stream events, median of 5 runs after 2 warm-ups with
the minimum and maximum; one JSON line.

The batch: --records x 1 kb records made on the device, records / 4 founders of random ACGT each followed by three copies with
1 % substitutions.  k = 21, 256 bins, 64 bands of 2 bins, threshold 0.2, min_filled 8.  One loop, alternating:

  sketch      circkit_sketch_batch_device + status over the batch (the yardstick of every other step)
  candidates  circkit_cluster_candidates_device + status: keys, resolve and emit together
  resolve     circkit_uniq_resolve_device alone, over the same keys (made here with torch from the rows, the definition restated
              in tensor arithmetic and held against the pairs the library finds)
  compare     circkit_sketch_compare_device + status over the candidate pairs
  link        circkit_cluster_link_device + status: init, link and flatten
  copy        circkit_bench_copy_device, the best of its variants

The C ABI has no call for the keys or the emit alone, so the two are reported together, as candidates minus resolve.  Every step
is reported against the sketch's time and against what a copy at the measured rate takes over the bytes the step moves.  The whole
circkit_cluster_batch from host memory is timed by the wall clock, 3 runs after 1.

    python tools/bench_cluster.py [--records N]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, K, LOG2_BINS, N_BANDS, BAND_BINS = 1000, 21, 8, 64, 2


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


def families_on_device(torch, ctx, dev, n, chunk=100_000):
    """n records of L symbols: record 4f is founder f, 4f + 1 .. 4f + 3 are copies of it with 1 % substitutions."""
    from circkit_amd import workloads
    founders, _ = workloads.fixed_length(ctx, dev, n // 4, L)
    ctx.synchronize()
    founders = founders[:n // 4 * L].view(n // 4, L)
    d_bytes = torch.empty(n * L + 64, dtype=torch.uint8, device=dev)
    out = d_bytes[:n * L].view(n, L)
    code = torch.zeros(256, dtype=torch.int64, device=dev)
    code[list(b"ACGT")] = torch.arange(4, device=dev)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev).manual_seed(7)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        rec = torch.arange(a, b, device=dev)
        src = founders[rec // 4]
        hit = (torch.rand((b - a, L), device=dev, generator=g) < 0.01) & (rec % 4 != 0)[:, None]
        other = acgt[(code[src.long()] + torch.randint(1, 4, (b - a, L), device=dev, generator=g)) % 4]
        out[a:b] = torch.where(hit, other, src)
    d_offs = (torch.arange(n + 1, dtype=torch.int64, device=dev) * L)
    return d_bytes, d_offs


def _s64(v):
    return v - 2 ** 64 if v >= 2 ** 63 else v


def fmix64(torch, h):
    for c in (0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53):
        h = (h ^ ((h >> 33) & 0x7FFFFFFF)) * _s64(c)
    return h ^ ((h >> 33) & 0x7FFFFFFF)


def keys_with_torch(torch, d_rows, n, dev, chunk=250_000):
    """The band keys of include/circkit.h in int64 tensor arithmetic (wrapping products, the logical shift spelled out)."""
    bins = 1 << LOG2_BINS
    rows = d_rows[:n * bins].view(n, bins)
    keys = torch.empty((n, N_BANDS), dtype=torch.int64, device=dev)
    seed = torch.tensor([_s64(((b + 1) * 0x9e3779b97f4a7c15) % 2 ** 64) for b in range(N_BANDS)], dtype=torch.int64, device=dev)
    for a in range(0, n, chunk):
        r = rows[a:a + chunk, :N_BANDS * BAND_BINS].reshape(-1, N_BANDS, BAND_BINS)
        x = seed[None, :].expand(r.shape[0], N_BANDS)
        for j in range(BAND_BINS):
            x = fmix64(torch, x ^ r[:, :, j])
        keys[a:a + chunk] = torch.where((r == -1).any(dim=2), torch.full_like(x, -1), x)
    return keys.view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_cluster: no HIP device")
    import circkit_amd
    from circkit_amd import api
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.records // 4 * 4
    bins = 1 << LOG2_BINS
    d_bytes, d_offs = families_on_device(torch, ctx, dev, n)
    sp = api.sketch_params(k=K, log2_bins=LOG2_BINS)
    cp = api.cluster_params(n_bands=N_BANDS, band_bins=BAND_BINS, min_similarity=0.2, min_filled=8)
    cap = n * N_BANDS
    d_rows = torch.empty(n * bins, dtype=torch.int64, device=dev)
    d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_pairs = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    d_scores = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    d_labels = torch.empty(n, dtype=torch.int64, device=dev)
    d_first = torch.empty(cap, dtype=torch.int64, device=dev)
    d_copy = torch.empty(n * L, dtype=torch.uint8, device=dev)
    ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows, params=sp)
    ctx.sketch_status()
    d_keys = keys_with_torch(torch, d_rows, n, dev)
    ctx.cluster_candidates_device(d_rows, n, LOG2_BINS, d_pair_off, d_pairs, cap, params=cp)
    n_pairs = ctx.cluster_candidates_status()
    # the keys made here are the library's: the same representatives give the same number of (rep < i) positions or more
    ctx.uniq_resolve_device(d_keys, cap, 0, d_first)
    ctx.uniq_status()
    pos = torch.arange(cap, device=dev)
    proposing = int(((d_first // N_BANDS < pos // N_BANDS) & (d_keys != -1)).sum())
    del pos
    assert proposing >= n_pairs > 0, (proposing, n_pairs)

    half = n * L // 16 * 16
    copies = {v: statistics.median(event_loop(torch, {"c": lambda v=v: ctx.bench_copy_device(d_bytes, d_copy, half, v)}, 3, 1)["c"]) for v in range(5)}
    best = min(copies, key=copies.get)
    t = event_loop(torch, {
        "sketch": lambda: (ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows, params=sp), ctx.sketch_status)[1],
        "candidates": lambda: (ctx.cluster_candidates_device(d_rows, n, LOG2_BINS, d_pair_off, d_pairs, cap, params=cp), ctx.cluster_candidates_status)[1],
        "resolve": lambda: (ctx.uniq_resolve_device(d_keys, cap, 0, d_first), ctx.uniq_status)[1],
        "compare": lambda: (ctx.sketch_compare_device(d_rows, n, d_rows, n, LOG2_BINS, d_pairs, n_pairs, d_scores), ctx.sketch_compare_status)[1],
        "link": lambda: (ctx.cluster_link_device(n, d_pairs, d_scores, n_pairs, d_labels, params=cp), ctx.cluster_link_status)[1],
        "copy": lambda: ctx.bench_copy_device(d_bytes, d_copy, half, best)}, a.steps, a.warmup)
    n_clusters, n_linked, _ = ctx.cluster_link_status()
    labels = d_labels.cpu().numpy().view(np.uint64)
    med = {name: statistics.median(v) for name, v in t.items()}
    copy_rate = 2 * half / med["copy"]
    moved = {
        "sketch": n * L + (n + 1) * 8 + n * bins * 8,
        "candidates": n * N_BANDS * BAND_BINS * 8 + cap * 8 * 4 + n * 8 * 4 + n_pairs * 8,       # rows read; keys and positions written and read; masks, offsets; pairs
        "resolve": cap * 8 * 2,
        "compare": n_pairs * (2 * bins * 8 + 8 + 8),
        "link": n_pairs * 16 + n * (4 + 4 + 8),
    }
    out = {"records": n, "record_length": L, "k": K, "bins": bins, "n_bands": N_BANDS, "band_bins": BAND_BINS, "pairs": n_pairs, "clusters": n_clusters,
           "linked": n_linked, "founders_that_lead_their_family": int((labels[::4] == np.arange(0, n, 4, dtype=np.uint64)).sum()),
           "copy_variant": best, "copy_bytes_per_s": round(copy_rate), "copy": stats(t["copy"])}
    for name in ("sketch", "candidates", "resolve", "compare", "link"):
        out[name] = {**stats(t[name]), "bytes_moved": moved[name], "copy_time_for_bytes_ms": round(moved[name] / copy_rate * 1e3, 4),
                     "fraction_of_copy": round(moved[name] / copy_rate / med[name], 4), "over_sketch": round(med[name] / med["sketch"], 4)}
    out["keys_and_emit_ms"] = round((med["candidates"] - med["resolve"]) * 1e3, 4)
    del d_keys, d_first, d_copy, d_pairs, d_scores, d_rows

    # ---- the whole chain from host memory ----------------------------------------------------------------------------------------
    h_bytes, h_offs = d_bytes[:n * L].cpu().numpy(), d_offs.cpu().numpy().view(np.uint64)
    times = []
    for it in range(4):
        t0 = time.perf_counter()
        host_labels, host_clusters = ctx.cluster_batch(h_bytes, h_offs, k=K, log2_bins=LOG2_BINS, params=cp)
        if it >= 1:
            times.append(time.perf_counter() - t0)
    out["cluster_batch"] = {**stats(times), "over_sketch": round(statistics.median(times) / med["sketch"], 4),
                            "labels_agree": bool(np.array_equal(host_labels, labels) and host_clusters == n_clusters)}
    print(json.dumps(out), flush=True)
    ctx.close()
    if not out["cluster_batch"]["labels_agree"]:
        sys.exit("bench_cluster: the host form and the device calls disagree")


if __name__ == "__main__":
    main()
