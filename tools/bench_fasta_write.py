#!/usr/bin/env python3
"""Measures the device FASTA writer on 1 kb records whose headers have the lengths of the reference
fixture's (tests/golden/ref_examples/nim_cated/realistic_input.fasta).  One JSON line with
  (a) circkit_fasta_write_device + circkit_fasta_write_status on resident data (text with head spans, a CSR batch of bodies),
      stream events round the enqueue and the wait: GB/s of written text, and as a fraction of the best
      circkit_bench_copy_device variant over the same number of output bytes in this process (reported, not judged);
  (b) circkit_fasta_write_text from page-locked host buffers into page-locked memory, end to end (wall clock); beside it the
      resident write of (a) followed by the copy of the written text to page-locked memory;
  (c) the path without the device writer: the body batch and its offsets copied home to page-locked memory, then a one-thread
      C++ loop of memcpy calls per record (the shape of the CLI's writer), compiled here from a small host source (wall clock).
The variants alternate inside one loop; each figure is the median of --runs after --warmup, with the minimum and maximum of the
runs beside it.  (b) must not be slower than (c), where overlapping [min, max] ranges count as equal: the script exits 1 otherwise.

    python tools/bench_fasta_write.py [--gb 1.0] [--runs 5] [--warmup 2]
"""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_LOOP = r"""
#include <stdint.h>
#include <string.h>
extern "C" uint64_t write_loop(const uint8_t* text, const uint64_t* head, const uint8_t* body, const uint64_t* offsets, uint64_t n, uint8_t* out)
{
    uint8_t* p = out;
    for (uint64_t i = 0; i < n; ++i) {
        *p++ = '>';
        memcpy(p, text + head[2 * i], head[2 * i + 1]);
        p += head[2 * i + 1];
        *p++ = '\n';
        const uint64_t len = offsets[i + 1] - offsets[i];
        memcpy(p, body + offsets[i], len);
        p += len;
        *p++ = '\n';
    }
    return (uint64_t)(p - out);
}
"""


def fixture_head_lengths():
    import circkit_amd
    text = open(os.path.join(ROOT, "tests", "golden", "ref_examples", "nim_cated", "realistic_input.fasta"), "rb").read()
    return [len(h) for h, _ in circkit_amd.api.fasta_parse(text)[0]]


def make_input(total_bytes, seed=5):
    """About total_bytes of written text: a block of 1024 records of 1000 bases under headers of the fixture's lengths, repeated.
    Returns (text, head spans, body, body offsets, records): the text is the FASTA file the records came from."""
    rng = np.random.default_rng(seed)
    lens = fixture_head_lengths()
    parts, heads, at = [], [], 0
    bodies = []
    for i in range(1024):
        h = bytes(rng.integers(ord("a"), ord("z") + 1, size=lens[i % len(lens)], dtype=np.uint8))
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1000).tobytes()
        heads.append((at + 1, len(h)))
        rec = b">" + h + b"\n" + seq + b"\n"
        parts.append(rec)
        bodies.append(seq)
        at += len(rec)
    block = np.frombuffer(b"".join(parts), dtype=np.uint8)
    reps = max(1, total_bytes // len(block))
    n = 1024 * reps
    spans = np.tile(np.array(heads, dtype=np.uint64), (reps, 1))
    spans[:, 0] += np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(len(block)), 1024)
    body = np.tile(np.frombuffer(b"".join(bodies), dtype=np.uint8), reps)
    return np.tile(block, reps), spans, body, 1000 * np.arange(n + 1, dtype=np.uint64), n


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

    tmp = tempfile.mkdtemp(prefix="bench_fasta_write_")
    src, so = os.path.join(tmp, "write_loop.cpp"), os.path.join(tmp, "write_loop.so")
    open(src, "w").write(HOST_LOOP)
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, src])
    loop = ctypes.CDLL(so).write_loop
    loop.restype, loop.argtypes = ctypes.c_uint64, [ctypes.c_void_p] * 4 + [ctypes.c_uint64, ctypes.c_void_p]
    shutil.rmtree(tmp, ignore_errors=True)                # (the library stays mapped)

    text, spans, body, offs, n_rec = make_input(int(args.gb * 1e9))
    n_text, n_body = len(text), len(body)
    total = n_text                                        # the written text is the file the records came from
    pin = lambda nbytes: lib.circkit_host_alloc(max(int(nbytes), 1))
    h_text, h_head, h_body, h_off = pin(n_text), pin(16 * n_rec), pin(n_body), pin(8 * (n_rec + 1))
    for p, a in ((h_text, text), (h_head, spans), (h_body, body), (h_off, offs)):
        ctypes.memmove(p, a.ctypes.data, a.nbytes)
    h_out, h_out_off, h_body_home, h_off_home = pin(total), pin(8 * (n_rec + 1)), pin(n_body), pin(8 * (n_rec + 1))
    d_text, d_body = torch.from_numpy(text).to(dev), torch.from_numpy(body).to(dev)
    d_head, d_off = torch.from_numpy(spans.view(np.int64).reshape(-1)).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev)
    d_out = torch.empty(total + 64, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n_rec + 1, dtype=torch.int64, device=dev)
    as_tensor = lambda p, nbytes: torch.from_numpy(np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint8)), shape=(nbytes,)))
    t_out, t_body_home, t_off_home = as_tensor(h_out, total), as_tensor(h_body_home, n_body), as_tensor(h_off_home, 8 * (n_rec + 1))
    d_off_bytes = d_off.view(torch.uint8)

    def copy_home(dst, d_src, nbytes):
        dst[:nbytes].copy_(d_src[:nbytes])                # device to page-locked host memory; returns when the bytes are there

    def events(fn, after=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        if after:
            after()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    seen = {}

    def write_a():
        ctx.fasta_write_device(d_text, n_text, d_head, n_rec, n_rec, d_out, total, d_out_off, d_body=d_body, d_body_offsets=d_off)

    def wait_a():
        seen["a"] = ctx.fasta_write_status()

    def write_b():
        t = ctypes.c_uint64(0)
        rc = lib.circkit_fasta_write_text(ctx._h, h_text, n_text, h_head, None, n_rec, None, n_rec, None, h_body, h_off, n_rec, h_out, total, h_out_off,
                                          ctypes.byref(t))
        assert rc == 0, lib.circkit_last_error(ctx._h).decode()
        seen["b"] = t.value

    def write_b_resident():
        write_a()
        wait_a()
        copy_home(t_out, d_out, total)

    def write_c():
        copy_home(t_body_home, d_body, n_body)
        copy_home(t_off_home, d_off_bytes, 8 * (n_rec + 1))
        seen["c"] = loop(h_text, h_head, h_body_home, h_off_home, n_rec, h_out)

    copy_bytes = total & ~15                              # (the copy kernels move whole 16-byte granules)
    runs = {"a": [], "b": [], "b_resident": [], "c": [], "copy": [[] for _ in range(5)]}
    for k in range(args.warmup + args.runs):
        keep = k >= args.warmup
        for v in range(5):
            t = events(lambda v=v: ctx.bench_copy_device(d_text, d_out, copy_bytes, variant=v))
            if keep:
                runs["copy"][v].append(t)
        t = events(write_a, wait_a)
        if keep:
            runs["a"].append(t)
        t = wall(write_b)
        b_text = ctypes.string_at(h_out, 4096) + ctypes.string_at(h_out + total - 4096, 4096)
        if k == 0:                                        # the whole text once per path; a sample of it every round
            assert np.array_equal(t_out.numpy(), text), "circkit_fasta_write_text wrote another text"
        if keep:
            runs["b"].append(t)
        t = wall(write_b_resident)
        if keep:
            runs["b_resident"].append(t)
        t = wall(write_c)
        c_text = ctypes.string_at(h_out, 4096) + ctypes.string_at(h_out + total - 4096, 4096)
        if keep:
            runs["c"].append(t)
        assert seen["a"] == (total, 0) and seen["b"] == total == seen["c"] and b_text == c_text, seen
    # the written text is the input file, whichever path wrote it
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(h_out, ctypes.POINTER(ctypes.c_uint8)), shape=(total,)), text)
    assert np.array_equal(d_out[:total].cpu().numpy(), text)

    a, b, br, c = stats(runs["a"]), stats(runs["b"]), stats(runs["b_resident"]), stats(runs["c"])
    copies = [stats(ts) for ts in runs["copy"]]
    best = min(range(5), key=lambda v: copies[v]["median_ms"])
    copy = copies[best]
    gbps = lambda s, nbytes=total: round(nbytes / (s["median_ms"] * 1e-3) / 1e9, 2)
    not_slower = b["median_ms"] <= c["median_ms"] or (b["min_ms"] <= c["max_ms"] and c["min_ms"] <= b["max_ms"])
    row = {"records": n_rec, "text_bytes": total, "body_bytes": n_body,
           "a_device_write": dict(a, text_gbps=gbps(a), fraction_of_copy=round((copy["median_ms"] / copy_bytes) / (a["median_ms"] / total), 3)),
           "copy_device": dict(copy, variant=best, bytes=copy_bytes, gbps=gbps(copy, copy_bytes)),
           "b_write_text_pinned": dict(b, text_gbps=gbps(b)),
           "b_resident_write_plus_copy_home": dict(br, text_gbps=gbps(br)),
           "c_copy_home_plus_host_loop": dict(c, text_gbps=gbps(c)),
           "b_not_slower_than_c": bool(not_slower)}
    print(json.dumps(row), flush=True)
    ctx.close()
    for p in (h_text, h_head, h_body, h_off, h_out, h_out_off, h_body_home, h_off_home):
        lib.circkit_host_free(p)
    sys.exit(0 if not_slower else 1)


if __name__ == "__main__":
    main()
