#!/usr/bin/env python
"""Throughput of circkit_monomers_compact_device on one MI355X, and of the chain it closes: median of 5 runs after 2
warm-ups, per case one JSON line:

  rolling          200 000 x 1 kb rolling-circle records (monomer 150..700, 1 % substitutions), seed 10, identity 0.95
  rolling_mixed    rolling records of 200 b .. 20 kb
  random_keep_all  random 1 kb records under keep_all: nothing monomerizes, every record is written whole

Per case:
  compact     the five kernels of the compact + the stream wait, on end indices computed once
  gather      the same minus the compact of a batch that writes nothing (min_length beyond every record): decide, scan and
              the launches without a byte moved -- what is left is the gather
  copy        circkit_bench_copy_device (best of its variants) over the same B bytes: the same bytes moved with nothing to decide
  chain       monomerize -> compact -> status -> canonicalize_batch_device with xxh3 -> uniq_resolve_device + the wait, next to
              the sum of its parts timed one by one
  host_route  circkit_monomerize_batch + slicing in numpy + circkit_canonicalize_batch (bytes + xxh3) on the same batch

    python tools/bench_monomers.py [--records N] [--cases rolling,rolling_mixed,random_keep_all]
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
    ap.add_argument("--records", type=int, default=0, help="records per case (default: 200 000; 20 000 for rolling_mixed)")
    ap.add_argument("--cases", default="rolling,rolling_mixed,random_keep_all")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_monomers: no HIP device")
    import circkit_amd
    from tests import mono_sets as S
    dev = torch.device("cuda", 0)
    ctx = circkit_amd.Context(0)
    params = dict(seed_len=10, min_identity=0.95)
    for case in a.cases.split(","):
        flt = dict(keep_all=True) if case == "random_keep_all" else {}
        if case == "rolling":
            n = a.records or 200_000
            data, offs = S.rolling(2024, np.full(n, 1000, dtype=np.int64))
        elif case == "rolling_mixed":
            n = a.records or 20_000
            rng = np.random.default_rng(77)
            data, offs = S.rolling(2025, np.exp(rng.uniform(np.log(200), np.log(20000), size=n)).astype(np.int64))
        else:
            n = a.records or 200_000
            data, offs = S.random_records(2026, np.full(n, 1000, dtype=np.int64))
        nb = int(offs[-1])
        d_bytes = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
        d_end = torch.empty(n, dtype=torch.int32, device=dev)
        d_mono = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
        d_moff = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_src = torch.empty(n, dtype=torch.int64, device=dev)
        d_canon = torch.empty(nb + 64, dtype=torch.uint8, device=dev)
        d_hash = torch.empty(n, dtype=torch.int64, device=dev)
        d_fs = torch.empty(n, dtype=torch.int64, device=dev)
        p = circkit_amd.monomerize_params(**params)
        f = circkit_amd.monomer_filter(**flt)
        f_none = circkit_amd.monomer_filter(min_length=2 ** 40)
        torch.cuda.synchronize()

        def monomerize():
            ctx.monomerize_batch_device(d_bytes, d_offs, n, d_end, params=p)

        def compact(flt_=f):
            ctx.monomers_compact_device(d_bytes, d_offs, n, d_end, d_mono, d_moff, d_src, filter=flt_)

        def canonicalize(m):
            ctx.canonicalize_batch_device(d_mono, d_moff, m, out_bytes=d_canon, out_xxh3=d_hash)

        def uniq(m):
            ctx.uniq_resolve_device(d_hash, m, 0, d_fs)

        def chain():
            monomerize()
            compact()
            m_, _ = ctx.monomers_status()
            canonicalize(m_)
            uniq(m_)

        t_mono = timed(ctx, monomerize, a.steps, a.warmup)
        t_compact = timed(ctx, compact, a.steps, a.warmup)
        m, B = ctx.monomers_status()
        t_empty = timed(ctx, lambda: compact(f_none), a.steps, a.warmup)
        assert ctx.monomers_status() == (0, 0)
        compact()
        assert ctx.monomers_status() == (m, B)
        t_status = timed(ctx, ctx.monomers_status, a.steps, a.warmup)
        t_canon = timed(ctx, lambda: canonicalize(m), a.steps, a.warmup)
        t_uniq = timed(ctx, lambda: uniq(m), a.steps, a.warmup)
        t_chain = timed(ctx, chain, a.steps, a.warmup)
        copies = {}
        nb16 = B // 16 * 16
        for v in range(5):
            copies[v] = timed(ctx, lambda: ctx.bench_copy_device(d_mono, d_canon, nb16, v), a.steps, a.warmup) if nb16 else 0.0
        best = min(copies, key=copies.get)
        t_copy = copies[best]
        t_gather = max(t_compact - t_empty, 0.0)

        # the host route on the same batch: end indices home, slices in numpy, the monomers back through the host form
        def host_route():
            ends = ctx.monomerize_batch(data, offs, **params)
            keep = np.ones(n, dtype=bool) if flt else ends != circkit_amd.api.MONOMER_NONE
            lens = np.where(ends != circkit_amd.api.MONOMER_NONE, ends, (offs[1:] - offs[:-1]).astype(np.uint32)).astype(np.int64)[keep]
            moff = np.zeros(len(lens) + 1, dtype=np.uint64)
            moff[1:] = np.cumsum(lens)
            rec = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
            mono = data[offs[:-1][keep].astype(np.int64)[rec] + (np.arange(int(moff[-1]), dtype=np.int64) - moff[:-1].astype(np.int64)[rec])]
            return ctx.canonicalize_batch(mono, moff, want_bytes=True, want_xxh3=True), moff

        t0 = time.perf_counter()
        (host, moff) = host_route()
        t_host = time.perf_counter() - t0
        same = int(moff[-1]) == B and np.array_equal(host["bytes"], d_canon[:B].cpu().numpy()) and \
            np.array_equal(host["xxh3"], d_hash[:m].cpu().numpy().view(np.uint64))
        print(json.dumps({
            "case": case, "records": n, "input_bytes": nb, "written_records": m, "written_bytes": B,
            "compact_seconds": round(t_compact, 6), "compact_nothing_written_seconds": round(t_empty, 6), "gather_seconds": round(t_gather, 6),
            "gather_bytes_per_s": round(B / t_gather) if t_gather else None,
            "copy_seconds": round(t_copy, 6), "copy_variant": best, "copy_bytes_per_s": round(nb16 / t_copy) if t_copy else None,
            "gather_over_copy": round(t_gather / t_copy, 3) if t_copy else None,
            "monomerize_seconds": round(t_mono, 6), "status_seconds": round(t_status, 6), "canonicalize_xxh3_seconds": round(t_canon, 6),
            "uniq_resolve_seconds": round(t_uniq, 6), "sum_of_parts_seconds": round(t_mono + t_compact + t_status + t_canon + t_uniq, 6),
            "chain_seconds": round(t_chain, 6), "host_route_seconds": round(t_host, 4), "host_route_over_chain": round(t_host / t_chain, 1),
            "host_route_matches": bool(same)}), flush=True)
        del d_bytes, d_offs, d_end, d_mono, d_moff, d_src, d_canon, d_hash, d_fs
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()
