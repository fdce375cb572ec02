#!/usr/bin/env python
"""Time of the distance unit on one MI355X: the device-resident batch of tools/bench_cluster.py, stream events, median of 5 runs
after 2 warm-ups with the minimum and maximum; one JSON line.

The batch: --records x 1 kb records made on the device, records / 4 founders of random ACGT each followed by three copies with
1 % substitutions.  k = 21, 256 bins, 64 bands of 2 bins, threshold 0.2, min_filled 8, min_votes 4, max_distance 32.  One loop,
alternating:

  prealign            circkit_prealign_pairs_device + status over the cluster's own candidate pairs
  gather              circkit_windows_gather_device + status: the second record of every candidate pair cut at its window
  distance            circkit_distance_pairs_device + status over (first record, cut second record) of every candidate pair
  members_prealign    the pairs (label, record) of all records and their windows
  members_gather      all records cut at their windows
  members_distance    circkit_distance_pairs_device + status over (label, record) on the gathered batch
  self_distance       the same call over (record, record): two equal 1 kb records, the wave-wide round 0 alone

    python tools/bench_distance.py [--records N] [--max-distance W]
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
    ap.add_argument("--max-distance", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_distance: no HIP device")
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
    dp = api.distance_params(max_distance=a.max_distance)
    cap = n * N_BANDS
    d_rows = torch.empty(n * bins, dtype=torch.int64, device=dev)
    d_anchors = torch.empty(n * bins, dtype=torch.int32, device=dev)
    d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_pairs = torch.empty(2 * cap, dtype=torch.int32, device=dev)
    d_labels = torch.empty(n, dtype=torch.int64, device=dev)
    ctx.sketch_anchors_device(d_bytes, d_offs, n, d_rows, d_anchors, params=sp)
    ctx.sketch_status()
    ctx.cluster_candidates_device(d_rows, n, LOG2_BINS, d_pair_off, d_pairs, cap, params=cp)
    n_pairs = ctx.cluster_candidates_status()
    d_pairs = d_pairs[:2 * n_pairs].clone()
    d_scores = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    ctx.sketch_compare_device(d_rows, n, d_rows, n, LOG2_BINS, d_pairs, n_pairs, d_scores)
    ctx.sketch_compare_status()
    ctx.cluster_link_device(n, d_pairs, d_scores, n_pairs, d_labels, params=cp)
    ctx.cluster_link_status()
    # the candidate pairs: a window and a cut record per pair, pair p = (first record, p)
    d_votes = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    d_win = torch.empty(n_pairs * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_cut = torch.empty(n_pairs * L, dtype=torch.uint8, device=dev)
    d_cut_off = torch.empty(n_pairs + 1, dtype=torch.int64, device=dev)
    d_ab = torch.stack((d_pairs[0::2], torch.arange(n_pairs, dtype=torch.int64, device=dev).to(torch.int32)), dim=1).reshape(-1).contiguous()
    d_dist = torch.empty(n_pairs, dtype=torch.int32, device=dev)
    d_id = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    # the members: every record against its representative, on the gathered batch
    d_rep = torch.empty(2 * n, dtype=torch.int32, device=dev)
    d_rep_votes = torch.empty(2 * n, dtype=torch.int32, device=dev)
    d_rep_win = torch.empty(n * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_rep_cut = torch.empty(n * L, dtype=torch.uint8, device=dev)
    d_rep_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_rep_dist = torch.empty(n, dtype=torch.int32, device=dev)
    d_self = torch.arange(n, dtype=torch.int64, device=dev).to(torch.int32).repeat_interleave(2).contiguous()
    d_self_dist = torch.empty(n, dtype=torch.int32, device=dev)

    def members_prealign():
        ctx.prealign_pairs_of_labels_device(d_labels, n, d_rep)
        ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_rep, n, d_rep_win, d_rep_votes, params=pp)
        return ctx.prealign_status

    within = {}

    def distance(name, *args):
        def run():
            ctx.distance_pairs_device(*args, params=dp)

            def after():
                within[name] = ctx.distance_status()[0]
            return after
        return run

    t = event_loop(torch, {
        "prealign": lambda: (ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_pairs, n_pairs, d_win, d_votes, params=pp), ctx.prealign_status)[1],
        "gather": lambda: (ctx.windows_gather_device(d_bytes, d_offs, n, d_win, n_pairs, d_cut, n_pairs * L, d_cut_off), ctx.windows_status)[1],
        "distance": distance("distance", d_bytes, d_offs, n, d_cut, d_cut_off, n_pairs, d_ab, n_pairs, d_dist, d_id),
        "members_prealign": members_prealign,
        "members_gather": lambda: (ctx.windows_gather_device(d_bytes, d_offs, n, d_rep_win, n, d_rep_cut, n * L, d_rep_off), ctx.windows_status)[1],
        "members_distance": distance("members_distance", d_rep_cut, d_rep_off, n, d_rep_cut, d_rep_off, n, d_rep, n, d_rep_dist, None),
        "self_distance": distance("self_distance", d_bytes, d_offs, n, d_bytes, d_offs, n, d_self, n, d_self_dist, None)}, a.steps, a.warmup)
    med = {name: statistics.median(v) for name, v in t.items()}
    dist = d_dist.cpu().numpy().view(np.uint32)
    rep_dist = d_rep_dist.cpu().numpy().view(np.uint32)
    inside = dist[dist != api.DISTANCE_OVER]
    out = {"records": n, "record_length": L, "k": K, "bins": bins, "min_votes": MIN_VOTES, "max_distance": a.max_distance, "pairs": n_pairs,
           "pairs_within": within["distance"], "share_within": round(within["distance"] / max(n_pairs, 1), 4),
           "mean_distance_within": round(float(inside.mean()), 3) if len(inside) else None,
           "members_within": within["members_distance"], "members_share_within": round(within["members_distance"] / n, 4),
           "largest_member_distance": int(rep_dist[rep_dist != api.DISTANCE_OVER].max()), "self_all_zero": bool((d_self_dist == 0).all())}
    for name in t:
        out[name] = stats(t[name])
    out["distance_ns_per_pair"] = round(med["distance"] / max(n_pairs, 1) * 1e9, 3)
    out["members_distance_ns_per_pair"] = round(med["members_distance"] / n * 1e9, 3)
    out["self_distance_ns_per_pair"] = round(med["self_distance"] / n * 1e9, 3)
    out["prealign_ns_per_pair"] = round(med["prealign"] / max(n_pairs, 1) * 1e9, 3)
    out["distance_over_prealign"] = round(med["distance"] / med["prealign"], 4)
    print(json.dumps(out), flush=True)
    ctx.close()
    if within["self_distance"] != n:
        sys.exit("bench_distance: a record is not at distance 0 from itself")


if __name__ == "__main__":
    main()
