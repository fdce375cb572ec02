#!/usr/bin/env python
"""Time of the prealign unit's steps on one MI355X: the device-resident batch of tools/bench_cluster.py, stream events, median of 5
runs after 2 warm-ups with the minimum and maximum; one JSON line.

The batch: --records x 1 kb records made on the device, records / 4 founders of random ACGT each followed by three copies with
1 % substitutions.  k = 21, 256 bins, 64 bands of 2 bins, threshold 0.2, min_filled 8, min_votes 4.  One loop, alternating:

  sketch          circkit_sketch_batch_device + status over the batch
  sketch_anchors  circkit_sketch_anchors_device + status over the same batch: what the anchors cost on top
  compare         circkit_sketch_compare_device + status over the cluster's own candidate pairs
  prealign        circkit_prealign_pairs_device + status over the same pairs: it reads half as many bytes again as the compare
                  (the anchors) and sorts; the ratio to the compare is what to report
  members         circkit_prealign_pairs_of_labels_device + circkit_prealign_pairs_device over (label, record) of all records
  gather          circkit_windows_gather_device + status: all records cut at their windows
  write           circkit_fasta_write_device + status: all records under a head

    python tools/bench_prealign.py [--records N]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_cluster import BAND_BINS, K, L, LOG2_BINS, N_BANDS, event_loop, families_on_device, stats  # noqa: E402

MIN_VOTES = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_prealign: no HIP device")
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
    pp = api.prealign_params(k=K, log2_bins=LOG2_BINS, min_votes=MIN_VOTES)
    cap = n * N_BANDS
    d_rows = torch.empty(n * bins, dtype=torch.int64, device=dev)
    d_rows2 = torch.empty(n * bins, dtype=torch.int64, device=dev)
    d_anchors = torch.empty(n * bins, dtype=torch.int32, device=dev)
    d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_pairs = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    d_labels = torch.empty(n, dtype=torch.int64, device=dev)
    ctx.sketch_anchors_device(d_bytes, d_offs, n, d_rows, d_anchors, params=sp)
    ctx.sketch_status()
    ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows2, params=sp)
    ctx.sketch_status()
    rows_agree = bool(torch.equal(d_rows, d_rows2))
    del d_rows2
    ctx.cluster_candidates_device(d_rows, n, LOG2_BINS, d_pair_off, d_pairs, cap, params=cp)
    n_pairs = ctx.cluster_candidates_status()
    d_pairs = d_pairs[:2 * n_pairs].clone()
    d_scores = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    d_votes = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    d_win = torch.empty(n_pairs * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    ctx.sketch_compare_device(d_rows, n, d_rows, n, LOG2_BINS, d_pairs, n_pairs, d_scores)
    ctx.sketch_compare_status()
    ctx.cluster_link_device(n, d_pairs, d_scores, n_pairs, d_labels, params=cp)
    ctx.cluster_link_status()
    d_rep = torch.empty(2 * n, dtype=torch.int32, device=dev)
    d_rep_votes = torch.empty(2 * n, dtype=torch.int32, device=dev)
    d_rep_win = torch.empty(n * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cut = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_cut_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    head = b"record words"
    d_text = torch.from_numpy(np.frombuffer(head, dtype=np.uint8).copy()).to(dev)
    d_head = torch.tensor([0, len(head)], dtype=torch.int64, device=dev).repeat(n, 1).contiguous()
    out_cap = n * (L + len(head) + 3) + 16
    d_out = torch.empty(out_cap, dtype=torch.uint8, device=dev)
    d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)

    def members():
        ctx.prealign_pairs_of_labels_device(d_labels, n, d_rep)
        ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_rep, n, d_rep_win, d_rep_votes, params=pp)
        return ctx.prealign_status

    members()()
    t = event_loop(torch, {
        "sketch": lambda: (ctx.sketch_batch_device(d_bytes, d_offs, n, d_rows, params=sp), ctx.sketch_status)[1],
        "sketch_anchors": lambda: (ctx.sketch_anchors_device(d_bytes, d_offs, n, d_rows, d_anchors, params=sp), ctx.sketch_status)[1],
        "compare": lambda: (ctx.sketch_compare_device(d_rows, n, d_rows, n, LOG2_BINS, d_pairs, n_pairs, d_scores), ctx.sketch_compare_status)[1],
        "prealign": lambda: (ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_pairs, n_pairs, d_win, d_votes, params=pp), ctx.prealign_status)[1],
        "members": members,
        "gather": lambda: (ctx.windows_gather_device(d_bytes, d_offs, n, d_rep_win, n, d_cut, n * L, d_cut_off), ctx.windows_status)[1],
        "write": lambda: (ctx.fasta_write_device(d_text, len(head), d_head, n, n, d_out, out_cap, d_out_off, d_body=d_cut, d_body_offsets=d_cut_off),
                          ctx.fasta_write_status)[1]}, a.steps, a.warmup)
    aligned, _ = ctx.prealign_status()                       # of the last prealign call of the loop: the members
    votes = d_rep_votes.cpu().numpy().view(np.uint32).reshape(n, 2)
    win = d_rep_win.cpu().numpy().view(api.WINDOW_DTYPE)
    med = {name: statistics.median(v) for name, v in t.items()}
    out = {"records": n, "record_length": L, "k": K, "bins": bins, "min_votes": MIN_VOTES, "pairs": n_pairs, "rows_agree": rows_agree,
           "members_aligned": aligned, "members_at_start_0_strand_0": int(((win["start"] == 0) & (win["strand"] == 0)).sum()),
           "fewest_votes_of_a_member": int(votes[:, 0].min())}
    for name in t:
        out[name] = stats(t[name])
    out["anchors_over_sketch"] = round(med["sketch_anchors"] / med["sketch"], 4)
    out["prealign_over_compare"] = round(med["prealign"] / med["compare"], 4)
    out["prealign_ns_per_pair"] = round(med["prealign"] / n_pairs * 1e9, 3)
    print(json.dumps(out), flush=True)
    ctx.close()
    if not rows_agree:
        sys.exit("bench_prealign: the anchors call and the plain sketch disagree on the rows")


if __name__ == "__main__":
    main()
