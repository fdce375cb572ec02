"""`circkit monomerize` (src/monomerize.rs:16-160) over the GPU batch call: the driver for in-memory FASTA text and a thin
`python -m circkit_amd.monomerize` wrapper for plain FASTA files and stdin / stdout.

    monomerize_fasta(text, **flags) -> (fasta_bytes, table_bytes or None)

The records and the normalized CSR batch come from api.fasta_parse, every record's end index from ONE
Context.monomerize_batch call; the worker's pre-check (src/monomerize.rs:80) and the writer closure (:90-150) are restated
here on the host, byte for byte: the head as read, the RAW sequence without line terminators (case kept), the table with
the csv crate's quoting.

The module itself is callable -- circkit_amd.monomerize(s, ...) is Monomerizer::monomerize[_sensitive] on one record
(api.monomerize) -- so that the package offers the lib-crate function and the driver under the name the reference uses
for both.
"""
import argparse
import os
import sys
import types

from . import api

NONE = api.MONOMER_NONE


def full_seq(raw):
    """seq_io Record::full_seq(): the sequence lines joined, their terminators (\\n, \\r\\n) removed."""
    return b"".join(line[:-1] if line.endswith(b"\r") else line for line in raw.split(b"\n"))


def csv_row(fields, delimiter):
    """A row as the csv crate writes it (QuoteStyle::Necessary): a field holding the delimiter, '"', '\\n' or '\\r' is
    quoted, its quotes doubled."""
    out = []
    for f in fields:
        if delimiter in f or b'"' in f or b"\n" in f or b"\r" in f:
            f = b'"' + f.replace(b'"', b'""') + b'"'
        out.append(f)
    return delimiter.join(out) + b"\n"


def monomerize_fasta(text, sensitive=False, seed_length=10, max_mismatch=None, min_identity=None, min_overlap=None,
                     min_overlap_percent=None, min_length=0, max_length=None, keep_all=False, table_delim=None, batch_fn=None):
    """The whole command on FASTA text.  table_delim: b"," or b"\\t" for a table, None for none (an empty table when no
    record is written, as the reference leaves an empty file).  batch_fn(data, offsets, seed_len=, max_mismatch=,
    min_identity=, sensitive=) -> uint32 end indices stands in for the default context's monomerize_batch.
    Raises ValueError for both cut-offs, a seed length outside 1..63, an identity outside [0, 1] or a FASTA format error."""
    api.monomerize_params(seed_length, max_mismatch, min_identity, sensitive)          # both cut-offs: ValueError
    if not 1 <= seed_length <= 63:
        raise ValueError("Seed length must be at least 1 and at most 63 but was set to %d." % seed_length)
    if min_identity is not None and not 0.0 <= min_identity <= 1.0:
        raise ValueError("min_identity must be between 0.0 and 1.0")
    recs, data, offs, _ = api.fasta_parse(text)
    if batch_fn is None:
        batch_fn = api.default_context().monomerize_batch
    ends = batch_fn(data, offs, seed_len=seed_length, max_mismatch=max_mismatch, min_identity=min_identity,
                    sensitive=sensitive) if recs else []
    out, rows = [], []
    for i, (head, raw) in enumerate(recs):
        n_norm = int(offs[i + 1] - offs[i])
        # the worker (src/monomerize.rs:80): a record shorter than the seed or than --min-length is not looked at
        idx = None if (n_norm < seed_length or n_norm < min_length or int(ends[i]) == NONE) else int(ends[i])
        full = full_seq(raw)
        # the writer (:97-125)
        if idx is not None and (idx < min_length or (max_length is not None and idx > max_length)):
            idx = None
        if min_overlap is not None and idx is not None and len(full) - idx < min_overlap:
            idx = None
        if min_overlap_percent is not None and idx is not None and float(len(full) - idx) / float(idx) < min_overlap_percent:
            idx = None                               # idx >= seed_length >= 1: the division is defined
        if idx is not None or keep_all:
            end = len(full) if idx is None else idx
            out.append(b">" + head + b"\n" + full[:end] + b"\n")
            if table_delim is not None:
                rows.append(csv_row([head, str(len(full)).encode(), str(end).encode()], table_delim))
    table = None
    if table_delim is not None:
        table = (table_delim.join([b"id", b"original_length", b"monomer_length"]) + b"\n" + b"".join(rows)) if rows else b""
    return b"".join(out), table


# ---------------------------------------------------------------------------------------------
# python -m circkit_amd.monomerize [INPUT] [-o OUT] [--table T] ...
# ---------------------------------------------------------------------------------------------
def _ranged_int(lo, hi):
    def parse(v):
        x = int(v)
        if not lo <= x <= hi:
            raise argparse.ArgumentTypeError("%s is not in %d..=%d" % (v, lo, hi))
        return x
    return parse


def _parser():
    p = argparse.ArgumentParser(prog="python -m circkit_amd.monomerize", description="Trim multimeric records to their first monomer")
    p.add_argument("input", nargs="?", help="input FASTA file [default: stdin]")
    p.add_argument("-o", "--output", help="output FASTA file [default: stdout]")
    p.add_argument("--sensitive", action="store_true")
    p.add_argument("--seed-length", type=_ranged_int(5, 64), default=10)
    p.add_argument("--max-mismatch", type=_ranged_int(0, 2 ** 64 - 1))
    p.add_argument("--min-identity", type=float)
    p.add_argument("--min-overlap", type=_ranged_int(0, 2 ** 64 - 1))
    p.add_argument("--min-overlap-percent", type=float)
    p.add_argument("--min-length", type=_ranged_int(0, 2 ** 64 - 1), default=0)
    p.add_argument("--max-length", type=_ranged_int(0, 2 ** 64 - 1))
    p.add_argument("-k", "--keep-all", action="store_true")
    p.add_argument("--table", help="id, original_length, monomer_length per written record; tab-separated for .tsv")
    p.add_argument("-t", "--threads", type=_ranged_int(0, 2 ** 32 - 1), help="accepted for the reference's command line; the GPU does the work")
    p.add_argument("--batch-size", type=_ranged_int(0, 2 ** 64 - 1), help=argparse.SUPPRESS)
    return p


def main(argv=None):
    """Exit status as the reference's: 2 for a bad flag value or both cut-offs, 1 for an identity outside [0, 1] or an
    unreadable input, 101 for --seed-length 64 (the builder's panic)."""
    p = _parser()
    a = p.parse_args(argv)
    if a.max_mismatch is not None and a.min_identity is not None:
        p.error("the argument '--max-mismatch <MAX_MISMATCH>' cannot be used with '--min-identity <MIN_IDENTITY>'")
    if a.min_identity is not None and not 0.0 <= a.min_identity <= 1.0:
        sys.stderr.write("Error: min_identity must be between 0.0 and 1.0\n")
        return 1
    try:
        if a.input is None:
            text = sys.stdin.buffer.read()
        else:
            with open(a.input, "rb") as f:
                text = f.read()
    except OSError as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    if a.seed_length == 64:
        sys.stderr.write("Seed length must be at least 1 and at most 63 but was set to 64.\n")
        return 101
    delim = None
    if a.table is not None:
        delim = b"\t" if os.path.splitext(a.table)[1] == ".tsv" else b","
    try:
        fasta, table = monomerize_fasta(text, sensitive=a.sensitive, seed_length=a.seed_length, max_mismatch=a.max_mismatch,
                                        min_identity=a.min_identity, min_overlap=a.min_overlap,
                                        min_overlap_percent=a.min_overlap_percent, min_length=a.min_length,
                                        max_length=a.max_length, keep_all=a.keep_all, table_delim=delim)
    except ValueError as e:
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


class _CallableModule(types.ModuleType):
    def __call__(self, s, **kw):
        return api.monomerize(s, **kw)


if __name__ == "__main__":
    sys.exit(main())
else:
    sys.modules[__name__].__class__ = _CallableModule
