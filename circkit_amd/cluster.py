"""`cluster`, the first open item of the reference's roadmap, as a driver over the device calls: the driver for in-memory FASTA
text and a thin `python -m circkit_amd.cluster` wrapper for plain FASTA files and stdin / stdout.

    cluster_fasta(text, **flags) -> (fasta_bytes, table_bytes, labels)

Nothing but the text goes to the device and nothing but the result comes back: the text is parsed there
(circkit_fasta_parse_device), every record sketched (circkit_sketch_batch_device), the candidate pairs made from the bands of
the rows (circkit_cluster_candidates_device), scored (circkit_sketch_compare_device) and linked (circkit_cluster_link_device);
the labels are a first_seen array, so circkit_uniq_compact_device packs the representatives and lists the members, and
circkit_fasta_write_device writes the representatives under their own heads with their normalized sequence.  The table names
every member that is not its cluster's representative: `member<TAB>representative`, the first word of either head, under a
title row of those two words, in input order.

With min_identity = F and max_distance = W (`--min-identity F --max-distance W`; both or neither) the pairs are linked on their
true identity instead of the sketch estimate: the one sketch also writes its anchors (circkit_sketch_anchors_device), every
candidate pair (a, b) gets the window that rotates and flips b onto a (circkit_prealign_pairs_device), the windows are cut into
a batch of their own (circkit_windows_gather_device), and circkit_distance_pairs_device gives the bounded edit distance d of a
and the cut b with L the longer of the two.  A pair links iff d <= W and 1 - d / L >= F (F kept as the nearest multiple of
2^-16).  A caller who wants F to decide alone picks W >= (1 - F) * the longest record, up to 255.  The rest of the chain, the
output and the table are the same.
"""
import argparse
import sys

import numpy as np

from . import api


def _word(head):
    parts = head.split(None, 1)
    return parts[0] if parts else b""


def cluster_fasta(text, k=21, log2_bins=8, seed=0, n_bands=64, band_bins=2, min_similarity=0.2, min_filled=8, min_identity=None, max_distance=None,
                  ctx=None):
    """The whole chain on FASTA text: (the representatives as FASTA, the member table, the labels as a uint64 array).  Raises
    ValueError on a FASTA format error, CirckitError on parameters out of range.  min_identity and max_distance (both or neither):
    link on the true identity of the pre-aligned pair, see above."""
    import torch
    if (min_identity is None) != (max_distance is None):
        raise ValueError("min_identity and max_distance go together")
    by_identity = min_identity is not None
    text = bytes(text)
    ctx = ctx or api.default_context()
    p = api.cluster_params(n_bands=n_bands, band_bins=band_bins, min_similarity=min_similarity, min_filled=min_filled)
    sp = api.sketch_params(k=k, log2_bins=log2_bins, seed=seed)
    title = b"member\trepresentative\n"
    n_text = len(text)
    if n_text == 0:
        return b"", title, np.zeros(0, dtype=np.uint64)
    dev = torch.device("cuda", ctx.device)
    cap_r = (n_text + 1) // 2
    with torch.cuda.device(dev):
        d_text = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
        d_data = torch.empty(n_text, dtype=torch.uint8, device=dev)
        d_offs = torch.empty(cap_r + 1, dtype=torch.int64, device=dev)
        d_spans = torch.empty((2, cap_r, 2), dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()             # the copies are torch's, the kernels the ctx stream's
        ctx.fasta_parse_device(d_text, n_text, d_data, n_text, d_offs, cap_r, d_spans[0], d_spans[1])
        try:
            n, n_bytes, _ = ctx.fasta_parse_status()
        except api.CirckitError as e:
            if "FASTA parse error" in str(e):                   # as fasta_parse reports it
                raise ValueError(str(e))
            raise
        if n == 0:
            return b"", title, np.zeros(0, dtype=np.uint64)
        d_rows = torch.empty(n << sp.log2_bins, dtype=torch.int64, device=dev)
        capacity = n * p.n_bands
        d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_pairs = torch.empty(2 * capacity, dtype=torch.int32, device=dev)
        d_scores = torch.empty(2 * capacity, dtype=torch.int32, device=dev)
        d_labels = torch.empty(n, dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        if by_identity:
            d_anchors = torch.empty(n << sp.log2_bins, dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()
            ctx.sketch_anchors_device(d_data, d_offs, n, d_rows, d_anchors, params=sp)
        else:
            ctx.sketch_batch_device(d_data, d_offs, n, d_rows, params=sp)
        ctx.cluster_candidates_device(d_rows, n, sp.log2_bins, d_pair_off, d_pairs, capacity, params=p)
        n_pairs = ctx.cluster_candidates_status()              # the compare takes the number of pairs from the host
        if by_identity:
            _identity_scores(ctx, dev, d_data, d_offs, n, d_rows, d_anchors, sp, d_pairs, n_pairs, d_scores, max_distance)
            p = api.cluster_params(n_bands=n_bands, band_bins=band_bins, min_similarity=min_identity, min_filled=1)
        else:
            ctx.sketch_compare_device(d_rows, n, d_rows, n, sp.log2_bins, d_pairs, n_pairs, d_scores)
        ctx.cluster_link_device(n, d_pairs, d_scores, n_pairs, d_labels, params=p)
        d_kept = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=dev)
        d_kept_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_src = torch.empty(n, dtype=torch.int64, device=dev)
        d_dup = torch.empty((2, n), dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        ctx.uniq_compact_device(d_data, d_offs, n, d_labels, d_kept, d_kept_off, d_src, 0, d_dup[0], d_dup[1])
        ctx.sketch_status()
        if not by_identity:
            ctx.sketch_compare_status()
        n_clusters, _, _ = ctx.cluster_link_status()
        m, kept_bytes = ctx.uniq_compact_status()
        assert m == n_clusters
        cap = n_text + kept_bytes + 2 * m + 16                 # every head lies in the text
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_out_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        ctx.fasta_write_device(d_text, n_text, d_spans[0], n, m, d_out, cap, d_out_off, d_body=d_kept, d_body_offsets=d_kept_off, d_src=d_src, n_src=m)
        total, _ = ctx.fasta_write_status()
        fasta = d_out[:total].cpu().numpy().tobytes()
        labels = d_labels.cpu().numpy().view(np.uint64).copy()
        dup = d_dup[:, :n - m].cpu().numpy().view(np.uint64)
        head = d_spans[0, :n].cpu().numpy().view(np.uint64)
    words = {}

    def word(i):
        if i not in words:
            words[i] = _word(text[int(head[i][0]):int(head[i][0] + head[i][1])])
        return words[i]

    table = title + b"".join(word(int(a)) + b"\t" + word(int(b)) + b"\n" for a, b in zip(dup[0], dup[1]))
    return fasta, table, labels


def _identity_scores(ctx, dev, d_data, d_offs, n, d_rows, d_anchors, sp, d_pairs, n_pairs, d_scores, max_distance):
    """d_scores[2p], d_scores[2p + 1] = (L - d, L) of candidate pair p = (a, b): d the bounded edit distance of record a and of
    record b cut by the window that puts it onto a.  Everything stays on the device; the host learns the size of the cut batch."""
    import torch
    if n_pairs == 0:
        return
    pp = api.prealign_params(k=sp.k, log2_bins=sp.log2_bins)
    d_win = torch.empty(n_pairs * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_votes = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    second = d_pairs[1:2 * n_pairs:2].to(torch.int64) & 0xFFFFFFFF                 # (the status has waited: the pairs are there)
    lengths = d_offs[1:n + 1] - d_offs[:n]
    cut_bytes = int(lengths[second].sum().item())             # every window is as long as its record
    d_cut = torch.empty(max(cut_bytes, 1), dtype=torch.uint8, device=dev)
    d_cut_off = torch.empty(n_pairs + 1, dtype=torch.int64, device=dev)
    d_ab = torch.stack((d_pairs[0:2 * n_pairs:2], torch.arange(n_pairs, dtype=torch.int64, device=dev).to(torch.int32)), dim=1).reshape(-1).contiguous()
    torch.cuda.current_stream().synchronize()
    ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_pairs, n_pairs, d_win, d_votes, params=pp)
    ctx.windows_gather_device(d_data, d_offs, n, d_win, n_pairs, d_cut, cut_bytes, d_cut_off)
    ctx.distance_pairs_device(d_data, d_offs, n, d_cut, d_cut_off, n_pairs, d_ab, n_pairs, None, d_scores, max_distance=max_distance)
    ctx.prealign_status()
    ctx.windows_status()
    ctx.distance_status()


# ---------------------------------------------------------------------------------------------
# python -m circkit_amd.cluster [-i INPUT] [-o OUT] [--table T] ...
# ---------------------------------------------------------------------------------------------
def _parser():
    p = argparse.ArgumentParser(prog="python -m circkit_amd.cluster", description="Cluster circular records by their k-mer sketches; write one representative per cluster")
    p.add_argument("-i", "--input", help="input FASTA file [default: stdin]")
    p.add_argument("-o", "--output", help="output FASTA file of the representatives [default: stdout]")
    p.add_argument("--k", type=int, default=21, help="k-mer length, 4 .. 32")
    p.add_argument("--bins", type=int, default=256, help="bins of a sketch: a power of two, 16 .. 1024")
    p.add_argument("--bands", type=int, default=64, help="bands of a row, 1 .. 64")
    p.add_argument("--band-bins", type=int, default=2, help="bins of a band, 1 .. 16")
    p.add_argument("--min-similarity", type=float, default=0.2, help="a pair links at match / filled of at least this")
    p.add_argument("--min-identity", type=float, default=None,
                   help="with --max-distance: link on the true identity 1 - d / L of the pre-aligned pair instead of the sketch estimate")
    p.add_argument("--max-distance", type=int, default=None, help="with --min-identity: the edit distance d is computed up to this, 0 .. 255; a pair beyond it does not link")
    p.add_argument("--table", help="member<TAB>representative for every record that is not its cluster's representative")
    return p


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    if a.bins < 1 or a.bins & (a.bins - 1):
        p.error("--bins must be a power of two")
    if (a.min_identity is None) != (a.max_distance is None):
        p.error("--min-identity and --max-distance go together")
    try:
        if a.input is None:
            text = sys.stdin.buffer.read()
        else:
            with open(a.input, "rb") as f:
                text = f.read()
    except OSError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    try:
        fasta, table, _ = cluster_fasta(text, k=a.k, log2_bins=a.bins.bit_length() - 1, n_bands=a.bands, band_bins=a.band_bins,
                                        min_similarity=a.min_similarity, min_identity=a.min_identity, max_distance=a.max_distance)
    except (ValueError, api.CirckitError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    if a.output is None:
        sys.stdout.buffer.write(fasta)
        sys.stdout.buffer.flush()
    else:
        with open(a.output, "wb") as f:
            f.write(fasta)
    if a.table is not None:
        with open(a.table, "wb") as f:
            f.write(table)
    return 0


if __name__ == "__main__":
    sys.exit(main())
