#!/usr/bin/env python3
"""Measures the device FASTA parser on text of 1 kb records in three forms: single-line FASTA, 80-column
FASTA, 80-column CRLF.  Per form, one JSON line with
  (a) circkit_fasta_parse_device + circkit_fasta_parse_status on resident text, stream events round the enqueue and the wait:
      GB/s of text, and as a fraction of what circkit_bench_copy_device moves for the same bytes in this process;
  (b) circkit_fasta_parse_text from page-locked host text into page-locked host buffers, end to end (wall clock);
  (c) the path without the device parser for the same batch: circkit_fasta_parse on one thread plus the copy of its packed
      batch (bytes and offsets) to the device (wall clock).
Each is the median of --runs after --warmup, with the minimum and maximum of the runs beside it.  (b) must not be slower than
(c): the script says so per form and exits 1 otherwise.

    python tools/bench_fasta_device.py [--gb 1.0] [--runs 5] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_text(form, total_bytes, seed=5):
    """About total_bytes of 1 kb records: a block of 1024 different records, repeated."""
    rng = np.random.default_rng(seed)
    eol = b"\r\n" if form == "crlf80" else b"\n"
    width = 0 if form == "single" else 80
    parts = []
    for i in range(1024):
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1000).tobytes()
        parts.append(b">read_%04d length=1000" % i + eol)
        if width:
            parts.extend(seq[a:a + width] + eol for a in range(0, 1000, width))
        else:
            parts.append(seq + eol)
    block = np.frombuffer(b"".join(parts), dtype=np.uint8)
    reps = max(1, total_bytes // len(block))
    return np.tile(block, reps), 1024 * reps


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(1e3 * ts[len(ts) // 2], 3), "min_ms": round(1e3 * ts[0], 3), "max_ms": round(1e3 * ts[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import circkit_amd
    if not torch.cuda.is_available():
        sys.exit("no HIP device: this benchmark measures the GPU")
    lib = circkit_amd.load_library()
    ctx = circkit_amd.Context(0)
    dev = torch.device("cuda", 0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ok = True
    rows = []
    for form in ("single", "wrap80", "crlf80"):
        text, n_rec = make_text(form, int(args.gb * 1e9))
        n = len(text)
        # page-locked host text and outputs
        pin = lambda nbytes: lib.circkit_host_alloc(max(int(nbytes), 1))
        h_text = pin(n)
        ctypes.memmove(h_text, text.ctypes.data, n)
        h_out, h_off, h_head, h_raw = pin(n), pin(8 * (n_rec + 1)), pin(16 * n_rec), pin(16 * n_rec)
        d_text = torch.from_numpy(text).to(dev)
        d_out = torch.empty(n, dtype=torch.uint8, device=dev)
        d_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
        d_spans = torch.empty((2, n_rec, 2), dtype=torch.int64, device=dev)

        def timed_events(fn, after=None):
            ts = []
            for k in range(args.warmup + args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                if after:
                    after()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    ts.append(e0.elapsed_time(e1) * 1e-3)
            return ts

        def timed_wall(fn):
            ts = []
            for k in range(args.warmup + args.runs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                if k >= args.warmup:
                    ts.append(time.perf_counter() - t0)
            return ts

        # the yardstick: the best of the plain copy kernels on the same bytes
        copy = min((stats(timed_events(lambda v=v: ctx.bench_copy_device(d_text, d_out, n, variant=v))) for v in range(4)), key=lambda s: s["median_ms"])

        counts = {}

        def parse_a(spans):
            ctx.fasta_parse_device(d_text, n, d_out, n, d_off, n_rec, d_spans[0] if spans else None, d_spans[1] if spans else None)

        def wait_a():
            counts["a"] = ctx.fasta_parse_status()

        a = stats(timed_events(lambda: parse_a(True), wait_a))
        a_bare = stats(timed_events(lambda: parse_a(False), wait_a))

        def parse_b():
            r, b, used = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            rc = lib.circkit_fasta_parse_text(ctx._h, h_text, n, 1, 1, h_out, n, h_off, n_rec, h_head, h_raw, ctypes.byref(r), ctypes.byref(b),
                                              ctypes.byref(used))
            assert rc == 0, lib.circkit_last_error(ctx._h).decode()
            counts["b"] = (r.value, b.value, used.value)

        b = stats(timed_wall(parse_b))

        def parse_c():
            h, used = ctypes.c_void_p(), ctypes.c_size_t(0)
            rc = lib.circkit_fasta_parse(h_text, n, 1, 1, ctypes.byref(h), ctypes.byref(used))
            assert rc == 0
            r = lib.circkit_fasta_n_records(h)
            offs = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_offsets(h), ctypes.POINTER(ctypes.c_int64)), shape=(r + 1,))
            total = int(offs[-1])
            data = np.ctypeslib.as_array(ctypes.cast(lib.circkit_fasta_bytes(h), ctypes.POINTER(ctypes.c_uint8)), shape=(total,))
            d_out[:total].copy_(torch.from_numpy(data))
            d_off[:r + 1].copy_(torch.from_numpy(offs))
            torch.cuda.synchronize()
            counts["c"] = (r, total, used.value)
            lib.circkit_fasta_free(h)

        c = stats(timed_wall(parse_c))
        assert counts["a"] == counts["b"] == counts["c"] and counts["a"][0] == n_rec, counts
        gbps = lambda s: round(n / (s["median_ms"] * 1e-3) / 1e9, 2)
        row = {"form": form, "text_bytes": n, "records": n_rec, "payload_bytes": counts["a"][1],
               "a_device_parse": dict(a, text_gbps=gbps(a), fraction_of_copy=round(copy["median_ms"] / a["median_ms"], 3)),
               "a_without_spans": dict(a_bare, text_gbps=gbps(a_bare), fraction_of_copy=round(copy["median_ms"] / a_bare["median_ms"], 3)),
               "copy_device": dict(copy, text_gbps=gbps(copy)),
               "b_parse_text_pinned": dict(b, text_gbps=gbps(b)),
               "c_host_parse_plus_copy": dict(c, text_gbps=gbps(c)),
               "b_not_slower_than_c": b["median_ms"] <= c["median_ms"]}
        ok = ok and row["b_not_slower_than_c"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del d_text, d_out, d_off, d_spans
        for p in (h_text, h_out, h_off, h_head, h_raw):
            lib.circkit_host_free(p)
    print("| form | text | (a) parse ms (GB/s, of copy) | (a) no spans ms | copy ms | (b) text ms [min, max] | (c) host + copy ms [min, max] |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        a, ab, cp, b, c = r["a_device_parse"], r["a_without_spans"], r["copy_device"], r["b_parse_text_pinned"], r["c_host_parse_plus_copy"]
        print("| %s | %.2f GB | %.2f (%.0f, %.2f) | %.2f | %.2f | %.1f [%.1f, %.1f] | %.1f [%.1f, %.1f] |" % (
            r["form"], r["text_bytes"] / 1e9, a["median_ms"], a["text_gbps"], a["fraction_of_copy"], ab["median_ms"], cp["median_ms"],
            b["median_ms"], b["min_ms"], b["max_ms"], c["median_ms"], c["min_ms"], c["max_ms"]))
    ctx.close()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
