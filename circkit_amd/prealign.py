"""`prealign`, the second open item of the reference's roadmap, as a driver over the device calls: the driver for in-memory FASTA
text and a thin `python -m circkit_amd.prealign` wrapper for plain FASTA files and stdin / stdout.

    prealign_fasta(text, **flags) -> (fasta_bytes, table_bytes, labels)

Nothing but the text goes to the device and nothing but the result comes back: the text is parsed there
(circkit_fasta_parse_device), every record sketched ONCE with its anchors (circkit_sketch_anchors_device), the rows clustered as
circkit_amd/cluster.py does (candidates, compare, link), every record paired with its cluster's representative
(circkit_prealign_pairs_of_labels_device) and the rotation and strand that put it onto the representative found
(circkit_prealign_pairs_device); circkit_windows_gather_device cuts all n records, in input order, and circkit_fasta_write_device
writes each under its own head.  Representatives and records that did not reach min_votes come out as they went in.  The table
holds `record<TAB>representative<TAB>strand<TAB>start<TAB>votes<TAB>matches` for every record, the first word of either head,
under a title row of those six words.  With max_distance = W (`--max-distance W`) the table has a seventh column `distance`:
the bounded edit distance of the record as it comes out and its representative (circkit_distance_pairs_device on the gathered
batch), or `*` when it is more than W.
"""
import argparse
import sys

import numpy as np

from . import api

TITLE = b"record\trepresentative\tstrand\tstart\tvotes\tmatches\n"


def _word(head):
    parts = head.split(None, 1)
    return parts[0] if parts else b""


def prealign_fasta(text, k=21, log2_bins=8, seed=0, n_bands=64, band_bins=2, min_similarity=0.2, min_filled=8, min_votes=4, max_distance=None,
                   ctx=None):
    """The whole chain on FASTA text: (every record rotated onto its representative as FASTA, the table, the labels as a uint64
    array).  Raises ValueError on a FASTA format error, CirckitError on parameters out of range.  max_distance: the table's seventh
    column, see above."""
    import torch
    text = bytes(text)
    ctx = ctx or api.default_context()
    p = api.cluster_params(n_bands=n_bands, band_bins=band_bins, min_similarity=min_similarity, min_filled=min_filled)
    sp = api.sketch_params(k=k, log2_bins=log2_bins, seed=seed)
    pp = api.prealign_params(k=k, log2_bins=log2_bins, min_votes=min_votes)
    n_text = len(text)
    title = TITLE if max_distance is None else TITLE[:-1] + b"\tdistance\n"
    if max_distance is not None:
        dp = api.distance_params(max_distance=max_distance)
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
        d_anchors = torch.empty(n << sp.log2_bins, dtype=torch.int32, device=dev)
        capacity = n * p.n_bands
        d_pair_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        d_pairs = torch.empty(2 * capacity, dtype=torch.int32, device=dev)
        d_scores = torch.empty(2 * capacity, dtype=torch.int32, device=dev)
        d_labels = torch.empty(n, dtype=torch.int64, device=dev)
        d_rep_pairs = torch.empty(2 * n, dtype=torch.int32, device=dev)
        d_votes = torch.empty(2 * n, dtype=torch.int32, device=dev)
        d_win = torch.empty(n * api.WINDOW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_cut = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=dev)
        d_cut_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        ctx.sketch_anchors_device(d_data, d_offs, n, d_rows, d_anchors, params=sp)      # the one sketch: its rows serve the candidates too
        ctx.cluster_candidates_device(d_rows, n, sp.log2_bins, d_pair_off, d_pairs, capacity, params=p)
        n_pairs = ctx.cluster_candidates_status()              # the compare takes the number of pairs from the host
        ctx.sketch_compare_device(d_rows, n, d_rows, n, sp.log2_bins, d_pairs, n_pairs, d_scores)
        ctx.cluster_link_device(n, d_pairs, d_scores, n_pairs, d_labels, params=p)
        ctx.prealign_pairs_of_labels_device(d_labels, n, d_rep_pairs)
        ctx.prealign_pairs_device(d_rows, d_anchors, d_offs, n, d_rep_pairs, n, d_win, d_votes, params=pp)
        ctx.windows_gather_device(d_data, d_offs, n, d_win, n, d_cut, n_bytes, d_cut_off)
        if max_distance is not None:                            # a representative's own window is the identity: the cut batch holds both sides
            d_dist = torch.empty(n, dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()
            ctx.distance_pairs_device(d_cut, d_cut_off, n, d_cut, d_cut_off, n, d_rep_pairs, n, d_dist, None, params=dp)
        ctx.sketch_status()
        ctx.sketch_compare_status()
        ctx.cluster_link_status()
        ctx.prealign_status()
        cut_bytes, _ = ctx.windows_status()
        if max_distance is not None:
            ctx.distance_status()
        assert cut_bytes == n_bytes                             # every window is as long as its record
        cap = n_text + cut_bytes + 2 * n + 16                  # every head lies in the text
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream().synchronize()
        ctx.fasta_write_device(d_text, n_text, d_spans[0], n, n, d_out, cap, d_out_off, d_body=d_cut, d_body_offsets=d_cut_off)
        total, _ = ctx.fasta_write_status()
        fasta = d_out[:total].cpu().numpy().tobytes()
        labels = d_labels.cpu().numpy().view(np.uint64).copy()
        win = d_win.cpu().numpy().view(api.WINDOW_DTYPE)
        votes = d_votes.cpu().numpy().view(np.uint32).reshape(n, 2)
        head = d_spans[0, :n].cpu().numpy().view(np.uint64)
        dist = None if max_distance is None else d_dist.cpu().numpy().view(np.uint32)
    words = [_word(text[int(h[0]):int(h[0] + h[1])]) for h in head]
    last = [b""] * n if dist is None else [b"\t*" if d == api.DISTANCE_OVER else b"\t%d" % d for d in dist]
    table = title + b"".join(b"%s\t%s\t%d\t%d\t%d\t%d%s\n" % (words[i], words[int(labels[i])], win["strand"][i], win["start"][i], votes[i][0], votes[i][1],
                                                               last[i]) for i in range(n))
    return fasta, table, labels


# ---------------------------------------------------------------------------------------------
# python -m circkit_amd.prealign [-i INPUT] [-o OUT] [--table T] ...
# ---------------------------------------------------------------------------------------------
def _parser():
    p = argparse.ArgumentParser(prog="python -m circkit_amd.prealign",
                                description="Cluster circular records by their k-mer sketches; write every record rotated and flipped onto its cluster's representative")
    p.add_argument("-i", "--input", help="input FASTA file [default: stdin]")
    p.add_argument("-o", "--output", help="output FASTA file of all records, in input order [default: stdout]")
    p.add_argument("--k", type=int, default=21, help="k-mer length, 4 .. 32")
    p.add_argument("--bins", type=int, default=256, help="bins of a sketch: a power of two, 16 .. 1024")
    p.add_argument("--bands", type=int, default=64, help="bands of a row, 1 .. 64")
    p.add_argument("--band-bins", type=int, default=2, help="bins of a band, 1 .. 16")
    p.add_argument("--min-similarity", type=float, default=0.2, help="a pair links at match / filled of at least this")
    p.add_argument("--min-votes", type=int, default=4, help="a record is rotated when this many shared bins agree on one rotation and strand")
    p.add_argument("--max-distance", type=int, default=None,
                   help="add a column `distance` to the table: the edit distance of each record as written and its representative, 0 .. 255, `*` beyond")
    p.add_argument("--table", help="record, representative, strand, start, votes, matches for every record, tab separated")
    return p


def main(argv=None):
    p = _parser()
    a = p.parse_args(argv)
    if a.bins < 1 or a.bins & (a.bins - 1):
        p.error("--bins must be a power of two")
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
        fasta, table, _ = prealign_fasta(text, k=a.k, log2_bins=a.bins.bit_length() - 1, n_bands=a.bands, band_bins=a.band_bins,
                                         min_similarity=a.min_similarity, min_votes=a.min_votes, max_distance=a.max_distance)
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
