#!/usr/bin/env python
"""Throughput of circkit_monomerize_batch_device on one MI355X: median of 5 runs after 2 warm-ups of the call + a stream
wait, per case one JSON line:

  random     10M x 1 kb random records made on the device (synth_fill_device): the scan alone, nothing monomerizes
  rolling    2M x 1 kb rolling-circle records (monomer 150..700, 1 % substitutions), made on the host with a fixed seed
  rolling_mixed   rolling records of 200 b .. 2 kb
  rolling_sensitive   the rolling batch with the sensitive form

The yardstick is the C restatement (tests/mono_ref.c) on 16 threads in the same run, timed on a head slice of the batch and
scaled to the batch; the slice's answers are compared with the GPU's.  fraction_of_8TBps counts the algorithmic traffic:
L + 8 + 4 bytes per record (the record, its offset, its answer).

    python tools/bench_monomerize.py [--records N] [--cases random,rolling,...] [--head 100000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=0, help="records per case (default: 10M random, 2M rolling)")
    ap.add_argument("--cases", default="random,rolling,rolling_mixed,rolling_sensitive")
    ap.add_argument("--head", type=int, default=100000, help="records of the head slice the restatement is timed on")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_monomerize: no HIP device")
    import circkit_amd
    from tests import mono_ref as R
    from tests import mono_sets as S
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    kw = dict(seed_len=10, min_identity=0.95)
    for case in a.cases.split(","):
        sens = case == "rolling_sensitive"
        if case == "random":
            n, L = a.records or 10_000_000, 1000
            d_bytes = torch.empty(n * L + 64, dtype=torch.uint8, device=dev)
            d_offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
            ctx.synth_fill_device(12345, 0, n * L, d_bytes)
            ctx.fixed_offsets_device(0, L, n, d_offs)
            ctx.synchronize()
            nbytes = n * L
            h = min(a.head, n)
            head_offs = np.arange(h + 1, dtype=np.uint64) * L
            head_data = d_bytes[:h * L].cpu().numpy()
        else:
            n = a.records or 2_000_000
            rng = np.random.default_rng(77)
            lengths = np.full(n, 1000, dtype=np.int64) if case != "rolling_mixed" else rng.integers(200, 2001, size=n)
            data, offs = S.rolling(2024, lengths)
            nbytes = int(offs[-1])
            d_bytes = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
            d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
            h = min(a.head, n)
            head_offs, head_data = offs[:h + 1].copy(), data[:int(offs[h])]
        d_end = torch.empty(n, dtype=torch.int32, device=dev)
        p = circkit_amd.monomerize_params(sensitive=sens, **kw)
        times = []
        for it in range(a.warmup + a.steps):
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx.monomerize_batch_device(d_bytes, d_offs, n, d_end, params=p)
            ctx.synchronize()
            if it >= a.warmup:
                times.append(time.perf_counter() - t0)
        t = statistics.median(times)
        got = d_end[:h].cpu().numpy().view(np.uint32)
        t0 = time.perf_counter()
        exp = R.batch(head_data, head_offs, threads=16, sensitive=sens, **kw)
        t_ref = (time.perf_counter() - t0) * (n / h)
        traffic = nbytes + 12 * n
        print(json.dumps({"case": case, "records": n, "input_bytes": nbytes, "seconds": round(t, 6), "records_per_s": round(n / t),
                          "input_bytes_per_s": round(nbytes / t), "fraction_of_8TBps": round(traffic / t / 8e12, 4),
                          "monomerized_fraction_head": round(float((exp != R.NONE).mean()), 4),
                          "restatement_16_threads_seconds_scaled": round(t_ref, 4), "speedup_vs_restatement": round(t_ref / t, 2),
                          "head_records": h, "head_matches": bool(np.array_equal(got, exp))}), flush=True)
        del d_bytes, d_offs, d_end
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
