"""Measures `circkit orfs` on the GPU (circkit_orfs_batch_device) and prints one JSON line per case.

    python tools/bench_orfs.py [--records 10000000] [--steps 5] [--warmup 2] [--ref-records 200000]

Cases: device-resident synthetic 1 kb records with the CLI's default flags (both strands); the same records with the
flags of the reference's hyperfine.sh (--start-codons ATG,CTG,TTG --max-wraps 0 --include-stop --strand both); a 200 b -
2 kb length mix with default flags.  Each line reports records/s, input bytes/s as a fraction of the 8 TB/s HBM peak,
and the speedup over the C restatement of the reference (tests/orfs_ref.c) on 16 threads, timed on --ref-records
records of the same batch and scaled per record.  Then `circkit orfs` wall time on a FASTA of --cli-records 1 kb records
written to /dev/shm (default and hyperfine flags, output to /dev/shm), one JSON line each."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
DEFAULT = dict(min_length=75, require_stop=True, strands="both")
HYPERFINE = dict(min_length=75, require_stop=True, strands="both", start_codons=("ATG", "CTG", "TTG"), max_wraps=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ref-records", type=int, default=200_000)
    ap.add_argument("--cli-records", type=int, default=1_000_000)
    a = ap.parse_args()
    import torch
    import circkit_amd
    from tests import orfs_ref as R
    ctx = circkit_amd.Context(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    cases = [("1kb_default", 1000, DEFAULT), ("1kb_hyperfine_flags", 1000, HYPERFINE), ("mix_200b_2kb_default", None, DEFAULT)]
    for name, L, flags in cases:
        n = a.records
        if L:
            lens = np.full(n, L, dtype=np.uint64)
        else:
            n = a.records * 1000 // 1100           # the same input size as the 1 kb cases
            lens = rng.integers(200, 2001, size=n).astype(np.uint64)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens)
        nb = int(offs[-1])
        d_bytes = torch.empty(nb, dtype=torch.uint8, device=dev)
        ctx.synth_fill_device(7, 0, nb, d_bytes)
        d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_orf_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        p = circkit_amd.orf_params(**flags)
        ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, None, 0, params=p)
        try:
            ctx.orfs_status()
            total = 0
        except circkit_amd.CirckitError:
            total = int(d_orf_off[-1].item())
        cap = max(total, 1)
        d_orfs = torch.empty(cap * 24, dtype=torch.uint8, device=dev)
        times = []
        for it in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.orfs_batch_device(d_bytes, d_offs, n, d_orf_off, d_orfs, cap, params=p)
            total = ctx.orfs_status()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                times.append(dt)
        t = float(np.median(times))
        # the restatement on 16 threads, on the first ref_records records of the same bytes
        m = min(a.ref_records, n)
        host = d_bytes[:int(offs[m])].cpu().numpy()
        kw = dict(start_codons=flags.get("start_codons", ("ATG",)), min_length=flags["min_length"], require_stop=True,
                  max_wraps=flags.get("max_wraps", 3), strands=3, mode=0)
        t0 = time.perf_counter()
        eo, _ = R.orfs_batch(host, offs[:m + 1], threads=16, **kw)
        t_ref = (time.perf_counter() - t0) * n / m
        got_head = d_orf_off[:m + 1].cpu().numpy().astype(np.uint64)
        print(json.dumps({"case": name, "records": n, "input_bytes": nb, "orfs": int(total), "median_s": round(t, 6),
                          "records_per_s": round(n / t), "input_bytes_per_s": round(nb / t), "fraction_of_8TBps": round(nb / t / PEAK, 4),
                          "ref16_s_scaled": round(t_ref, 3), "speedup_vs_ref16": round(t_ref / t, 1),
                          "offsets_match_ref_on_head": bool(np.array_equal(got_head, eo))}), flush=True)
        del d_bytes, d_orfs, d_offs, d_orf_off
        torch.cuda.empty_cache()
    ctx.close()
    if a.cli_records:
        cli_wall(a.cli_records)


def cli_wall(n, L=1000):
    import subprocess
    from oracle import oracle as O
    shm = "/dev/shm/circkit_orfs_bench_%d" % os.getpid()
    os.makedirs(shm, exist_ok=True)
    path = os.path.join(shm, "in.fa")
    try:
        seq = O.synth_fill(3, 0, n * L).tobytes()
        with open(path, "wb") as f:
            step = 100_000
            for r0 in range(0, n, step):
                f.write(b"".join(b">r%d\n" % r + seq[r * L:(r + 1) * L] + b"\n" for r in range(r0, min(n, r0 + step))))
        size = os.path.getsize(path)
        binary = os.path.join(ROOT, "circkit_amd", "circkit")
        for name, flags in (("cli_default", []), ("cli_hyperfine_flags", ["--start-codons", "ATG,CTG,TTG", "--max-wraps", "0",
                                                                         "--include-stop", "--strand", "both"])):
            out = os.path.join(shm, "out.fa")
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([binary, "orfs", path, "-o", out] + flags, check=True)
                times.append(time.perf_counter() - t0)
            print(json.dumps({"case": name, "records": n, "input_file_bytes": size, "output_bytes": os.path.getsize(out),
                              "wall_s_median_of_3": round(float(np.median(times)), 3),
                              "records_per_s": round(n / float(np.median(times)))}), flush=True)
    finally:
        for f in os.listdir(shm):
            os.remove(os.path.join(shm, f))
        os.rmdir(shm)


if __name__ == "__main__":
    main()
