"""ctypes loader of tests/mono_ref.c (TEST INFRASTRUCTURE ONLY: the restatement of the reference's Monomerizer the GPU
kernel is checked against) plus a Python restatement of the `circkit monomerize` worker, writer and table
(src/monomerize.rs:16-160).

tests/libck_mono_ref.so is git-ignored; build() compiles it with gcc when it is missing or older than the source, and
__graft_entry__.build() calls it so that it travels to the GPU box with the tree."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "mono_ref.c")
LIB = os.path.join(HERE, "libck_mono_ref.so")

NONE = 0xFFFFFFFF
BOTH_SET = ("Both overlap_dist and overlap_min_identity are set. They are mutually exclusive since they may produce "
            "conflicting filtering results.")


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-Wall", "-Wextra", "-std=c11", "-ffp-contract=off", "-shared", "-o", LIB, SRC,
                               "-lpthread", "-lm"])
    return LIB


class Params(ctypes.Structure):
    _fields_ = [("seed_len", ctypes.c_uint32), ("use_identity", ctypes.c_uint32), ("overlap_dist", ctypes.c_uint64),
                ("min_identity", ctypes.c_double), ("sensitive", ctypes.c_uint32)]


def params(seed_len=10, max_mismatch=None, min_identity=None, sensitive=False):
    """MonomerizerBuilder: seed 1..63, one cut-off at most (overlap_dist defaults to 0)."""
    if max_mismatch is not None and min_identity is not None:
        raise ValueError(BOTH_SET)
    if not 1 <= int(seed_len) <= 63:
        raise ValueError("Seed length must be at least 1 and at most 63 but was set to %d." % seed_len)
    return Params(int(seed_len), int(min_identity is not None), int(max_mismatch or 0),
                  float(min_identity) if min_identity is not None else 0.0, int(bool(sensitive)))


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB)
        pp = ctypes.POINTER(Params)
        wp = ctypes.POINTER(ctypes.c_uint64)
        for name in ("ck_mono_ref_first", "ck_mono_ref_last", "ck_mono_ref_sensitive", "ck_mono_ref_end"):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_size_t, pp, wp]
        L.ck_mono_ref_sensitive_free.restype = ctypes.c_int64
        L.ck_mono_ref_sensitive_free.argtypes = [ctypes.c_void_p, ctypes.c_size_t, pp]
        L.ck_mono_ref_batch.restype = ctypes.c_uint64
        L.ck_mono_ref_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, pp, ctypes.c_void_p, ctypes.c_int]
        L.ck_mono_ref_set_complement.argtypes = [ctypes.c_void_p]
        # the sensitive form reverse-complements with the oracle's table (bio's dna::complement)
        from oracle import oracle as O
        tab = (ctypes.c_uint8 * 256)(*[O.lib().ck_oracle_complement(b) for b in range(256)])
        L.ck_mono_ref_set_complement(tab)
        _lib = L
    return _lib


def complement_table():
    from oracle import oracle as O
    return bytes(O.lib().ck_oracle_complement(b) for b in range(256))


def _call(fn, seq, p, want_work=False):
    seq = bytes(seq)
    buf = ctypes.create_string_buffer(seq, max(len(seq), 1))
    w = ctypes.c_uint64(0)
    r = fn(ctypes.addressof(buf), len(seq), ctypes.byref(p), ctypes.byref(w))
    r = None if r < 0 else int(r)
    return (r, w.value) if want_work else r


def first_end_index(seq, **kw):
    """first_monomer_end_index (one pass)."""
    return _call(lib().ck_mono_ref_first, seq, params(**kw))


def end_index(seq, want_work=False, **kw):
    """last_monomer_end_index, or its sensitive form with sensitive=True: an int or None."""
    return _call(lib().ck_mono_ref_end, seq, params(**kw), want_work)


def end_index_free(seq, **kw):
    """The sensitive form without a reverse complement (what the kernel computes)."""
    seq = bytes(seq)
    buf = ctypes.create_string_buffer(seq, max(len(seq), 1))
    p = params(**kw)
    r = lib().ck_mono_ref_sensitive_free(ctypes.addressof(buf), len(seq), ctypes.byref(p))
    return None if r < 0 else int(r)


def monomerize(seq, **kw):
    """Monomerizer::monomerize / monomerize_sensitive."""
    seq = bytes(seq)
    e = end_index(seq, **kw)
    return seq if e is None else seq[:e]


def batch(data, offsets, threads=4, want_work=False, **kw):
    """uint32 end index (NONE = None) of every record of a CSR batch."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    p = params(**kw)
    out = np.full(max(n, 1), NONE, dtype=np.uint32)
    base = data.ctypes.data if len(data) else None
    work = lib().ck_mono_ref_batch(base, offsets.ctypes.data, n, ctypes.byref(p), out.ctypes.data, int(threads))
    return (out[:n], int(work)) if want_work else out[:n]


# ---------------------------------------------------------------------------------------------
# `circkit monomerize` on an in-memory FASTA (src/monomerize.rs:16-160)
# ---------------------------------------------------------------------------------------------
def write_records(recs, ends, min_overlap=None, min_overlap_percent=None, min_length=0, max_length=None, keep_all=False,
                  table_delim=None):
    """The writer closure (src/monomerize.rs:90-150).  recs: [(head, full_seq)], ends: the worker's result per record (an
    int or None).  Returns (fasta_bytes, table_bytes | None); the table's fields are quoted as the csv crate does."""
    from oracle import oracle as O
    out, rows = [], []
    for (head, full), idx in zip(recs, ends):
        if idx is not None and (idx < min_length or (max_length is not None and idx > max_length)):
            idx = None
        if min_overlap is not None and idx is not None and len(full) - idx < min_overlap:
            idx = None
        if min_overlap_percent is not None and idx is not None:
            # (full_seq.len() - monomer_length) as f64 / (monomer_length as f64): x / 0.0 is inf or NaN, never below
            ratio = (float(len(full) - idx) / float(idx)) if idx else (float("inf") if len(full) else float("nan"))
            if ratio < min_overlap_percent:
                idx = None
        if idx is not None or keep_all:
            end = len(full) if idx is None else idx
            out.append(b">" + head + b"\n" + full[:end] + b"\n")
            if table_delim is not None:
                rows.append(O.csv_row([head, str(len(full)).encode(), str(end).encode()], table_delim))
    table = None
    if table_delim is not None:
        table = (table_delim.join([b"id", b"original_length", b"monomer_length"]) + b"\n" + b"".join(rows)) if rows else b""
    return b"".join(out), table


def cli_monomerize(data, sensitive=False, seed_length=10, max_mismatch=None, min_identity=None, min_overlap=None,
                   min_overlap_percent=None, min_length=0, max_length=None, keep_all=False, table_delim=None, threads=4):
    """Returns (fasta_bytes, table_bytes | None)."""
    from oracle import oracle as O
    kw = dict(seed_len=seed_length, max_mismatch=max_mismatch, min_identity=min_identity, sensitive=sensitive)
    params(**kw)
    recs, norms = [], []
    for head, raw in O.read_fasta(data):
        recs.append((head, O.full_seq(raw)))
        norms.append(O.normalize(raw)[0])
    offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in norms])
    joined = np.frombuffer(b"".join(norms) + b"\0", dtype=np.uint8)[:int(offs[-1])]
    got = batch(joined, offs, threads=threads, **kw)
    ends = []
    for norm, e in zip(norms, got):
        # the worker's pre-check (src/monomerize.rs:80): shorter than the seed or than --min-length
        ends.append(None if (len(norm) < seed_length or len(norm) < min_length or int(e) == NONE) else int(e))
    return write_records(recs, ends, min_overlap, min_overlap_percent, min_length, max_length, keep_all, table_delim)
