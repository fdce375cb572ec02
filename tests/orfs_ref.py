"""ctypes loader of tests/orfs_ref.c (TEST INFRASTRUCTURE ONLY: the restatement of the reference's ORF finder the GPU
kernels are checked against) plus a Python restatement of the `circkit orfs` writer and table (src/orfs.rs:106-191).

tests/libck_orfs_ref.so is git-ignored; build() compiles it with gcc when it is missing or older than the source, and
__graft_entry__.build() calls it so that it travels to the GPU box with the tree."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "orfs_ref.c")
LIB = os.path.join(HERE, "libck_orfs_ref.so")
LANE_SRC = os.path.join(HERE, "orfs_lane_host.cpp")
LANE_HDR = os.path.join(os.path.dirname(HERE), "circkit_amd", "csrc", "orfs.h")
LANE_LIB = os.path.join(HERE, "libck_orfs_lane.so")

NONE = 0xFFFFFFFF
ORF_DTYPE = np.dtype([("length", "<u8"), ("start", "<u4"), ("stop", "<u4"), ("wraps", "<u4"), ("strand", "<u4")])
DEFAULT_START = ("ATG",)
DEFAULT_STOP = ("TAA", "TAG", "TGA")


def build(force=False):
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-Wall", "-Wextra", "-std=c11", "-shared", "-o", LIB, SRC, "-lpthread"])
    return LIB


def build_lane(force=False):
    """The kernel's per-lane routine (circkit_amd/csrc/orfs.h) built for the host: tests/orfs_lane_host.cpp."""
    if force or not os.path.exists(LANE_LIB) or any(os.path.getmtime(LANE_LIB) < os.path.getmtime(f) for f in (LANE_SRC, LANE_HDR)):
        subprocess.check_call(["g++", "-O2", "-fPIC", "-std=c++17", "-Wall", "-shared", "-o", LANE_LIB, LANE_SRC])
    return LANE_LIB


class _Codons(ctypes.Structure):
    _fields_ = [("codons", ctypes.c_void_p), ("n", ctypes.c_int)]


class _Params(ctypes.Structure):
    _fields_ = [("start", _Codons), ("stop", _Codons), ("min_length", ctypes.c_uint64), ("min_ratio", ctypes.c_double),
                ("min_wraps", ctypes.c_uint32), ("max_wraps", ctypes.c_uint32), ("require_stop", ctypes.c_int),
                ("strand_mask", ctypes.c_int), ("mode", ctypes.c_int)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB)
        L.ck_ref_orfs_batch.restype = ctypes.c_uint64
        L.ck_ref_orfs_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int]
        L.ck_ref_find_orfs.restype = ctypes.c_size_t
        L.ck_ref_find_orfs.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
        L.ck_ref_init()
        _lib = L
    return _lib


def codon_bytes(codons):
    """The codons of a list that can ever match (the reference compares &str; a codon whose length is not 3 never does)."""
    out = [c.encode() if isinstance(c, str) else bytes(c) for c in codons]
    return b"".join(c for c in out if len(c) == 3)


def params(start_codons=DEFAULT_START, stop_codons=DEFAULT_STOP, min_length=0, min_ratio=0.0, min_wraps=0, max_wraps=3,
           require_stop=False, strands=3, mode=0):
    st, sp = codon_bytes(start_codons), codon_bytes(stop_codons)
    keep = [st, sp]                 # the structure points into these
    p = _Params(_Codons(ctypes.cast(ctypes.c_char_p(st), ctypes.c_void_p), len(st) // 3),
                _Codons(ctypes.cast(ctypes.c_char_p(sp), ctypes.c_void_p), len(sp) // 3),
                int(min_length), float(min_ratio), int(min_wraps), int(max_wraps), int(bool(require_stop)), int(strands), int(mode))
    p._keep = keep
    return p


def orfs_batch(data, offsets, threads=4, **kw):
    """Every record's ORFs (forward first, then reverse): (offsets[n + 1], structured array of ORF_DTYPE)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    p = params(**kw)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    base = data.ctypes.data if len(data) else None
    total = lib().ck_ref_orfs_batch(base, offsets.ctypes.data, n, ctypes.byref(p), out_off.ctypes.data, None, int(threads))
    out = np.zeros(max(total, 1), dtype=ORF_DTYPE)
    lib().ck_ref_orfs_batch(base, offsets.ctypes.data, n, ctypes.byref(p), out_off.ctypes.data, out.ctypes.data, int(threads))
    return out_off, out[:total]


_lane = None


def lane_orfs_batch(data, offsets, **kw):
    """orfs_batch through the kernel's per-lane routine on the host (same return shape)."""
    global _lane
    if _lane is None:
        build_lane()
        _lane = ctypes.CDLL(LANE_LIB)
        _lane.ck_lane_orfs_batch.restype = ctypes.c_uint64
        _lane.ck_lane_orfs_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64] + [ctypes.c_void_p] * 3
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    p = params(**kw)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    base = data.ctypes.data if len(data) else None
    total = _lane.ck_lane_orfs_batch(base, offsets.ctypes.data, n, ctypes.byref(p), out_off.ctypes.data, None)
    out = np.zeros(max(total, 1), dtype=ORF_DTYPE)
    _lane.ck_lane_orfs_batch(base, offsets.ctypes.data, n, ctypes.byref(p), out_off.ctypes.data, out.ctypes.data)
    return out_off, out[:total]


def orfs_record(seq, **kw):
    """[(start, stop|None, wraps, length, strand)] of one normalized record."""
    data = np.frombuffer(bytes(seq), dtype=np.uint8)
    _, o = orfs_batch(data, np.array([0, len(data)], dtype=np.uint64), threads=1, **kw)
    return [(int(r["start"]), None if int(r["stop"]) == NONE else int(r["stop"]), int(r["wraps"]), int(r["length"]), int(r["strand"]))
            for r in o]


def find_orfs(seq):
    """lib/src/orfs.rs:41 find_orfs: [(start, stop|None, wraps, length)] in the reference's order."""
    seq = bytes(seq)
    buf = ctypes.create_string_buffer(seq, max(len(seq), 1))
    cap = 3 * len(seq) + 8
    out = np.zeros(cap, dtype=ORF_DTYPE)
    n = lib().ck_ref_find_orfs(ctypes.addressof(buf), len(seq), out.ctypes.data, cap)
    return [(int(r["start"]), None if int(r["stop"]) == NONE else int(r["stop"]), int(r["wraps"]), int(r["length"])) for r in out[:n]]


# ---------------------------------------------------------------------------------------------
# `circkit orfs` on an in-memory FASTA (src/orfs.rs:25-192)
# ---------------------------------------------------------------------------------------------
def ryu_f64(x):
    """An f64 as the csv crate writes it (ryu): shortest round-trip digits, `1.0`, `0.5`, `0.00012`, `1e-7`, `1e16`."""
    r = repr(float(x))
    if "e" in r:
        m, e = r.split("e")
        if m.endswith(".0"):
            m = m[:-2]
        e = int(e)
        if -5 <= e < 16:            # ryu's plain range: 1e-5 .. 1e16 written out
            from decimal import Decimal
            return format(Decimal(repr(float(x))), "f") if e < 0 else str(int(float(x))) + ".0"
        return "%se%d" % (m, e)
    return r


def cyclic_cut(src, start, n):
    """Orf::seq: n bytes of src read cyclically from start (n may exceed len(src))."""
    if n <= 0 or not src:
        return b""
    s = start % len(src)
    parts = [src[s:s + n]]                                 # (collected and joined once: a window of half a million laps stays linear)
    have = len(parts[0])
    while have < n:
        parts.append(src[:n - have])
        have += len(parts[-1])
    return src[:0].join(parts)


def cli_orfs(data, min_length=75, start_codons="ATG", stop_codons="TAA,TAG,TGA", include_stop=False, no_stop_required=False,
             min_wraps=0, max_wraps=3, strand="both", min_ratio=0.0, table_delim=None, threads=16):
    """Returns (fasta_bytes, table_bytes|None).  Raises ValueError on a record of fewer than 2 symbols (the reference's
    panic).  Table fields are quoted as the csv crate does (oracle.csv_row)."""
    from oracle import oracle as O
    strands = 1 if strand == "forward" else 3          # --strand reverse prints both lists too (src/orfs.rs:79-103)
    kw = dict(start_codons=start_codons.split(","), stop_codons=stop_codons.split(","), min_length=min_length,
              min_ratio=min_ratio, min_wraps=min_wraps, max_wraps=max_wraps, require_stop=not no_stop_required,
              strands=strands, mode=0)
    recs = []
    for head, raw in O.read_fasta(data):
        norm, _ = O.normalize(raw)
        if len(norm) < 2:
            raise ValueError("record of %d symbols" % len(norm))
        recs.append((head, raw, norm))
    # the worker closure for every record at once (threaded), then the writer closure record by record
    norms = [r[2] for r in recs]
    offs = np.zeros(len(recs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(x) for x in norms])
    joined = np.frombuffer(b"".join(norms) + b"\0", dtype=np.uint8)[:int(offs[-1])]
    orf_off, orfs = orfs_batch(joined, offs, threads=threads, **kw)
    out, rows = [], []
    cut = 0 if include_stop else 3
    for i, (head, raw, norm) in enumerate(recs):
        o0, o1 = int(orf_off[i]), int(orf_off[i + 1])
        if o0 == o1:
            continue
        full = O.full_seq(raw)
        rc = O.revcomp(norm)
        L = len(norm)
        for r in orfs[o0:o1]:
            start, length, wraps, st = int(r["start"]), int(r["length"]), int(r["wraps"]), int(r["strand"])
            stop = None if int(r["stop"]) == NONE else int(r["stop"])
            src = full if st == 0 else rc
            seq = cyclic_cut(src, start, length - cut)
            tag = b"_ORF" if st == 0 else b"_RC_ORF"
            orf_id = head + tag + str(start).encode()
            out.append(b">" + orf_id + b"\n" + seq + b"\n")
            if table_delim is not None:
                if st == 1:
                    t_start, t_stop = L - 1 - start, (None if stop is None else L - 1 - stop)
                else:
                    t_start, t_stop = start, stop
                fields = [orf_id, head, str(t_start).encode(), b"" if t_stop is None else str(t_stop).encode(),
                          str(length - cut).encode(), str(wraps).encode(), ryu_f64(length / len(full)).encode()]
                rows.append(O.csv_row(fields, table_delim))
    table = None
    if table_delim is not None:
        table = (table_delim.join([b"orf_id", b"seq_id", b"start", b"stop", b"length", b"wraps", b"ratio"]) + b"\n" +
                 b"".join(rows)) if rows else b""
    return b"".join(out), table
