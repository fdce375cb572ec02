"""Plain numpy / bytes restatement of the cyclic windows of include/circkit.h (TEST INFRASTRUCTURE ONLY): what
circkit_windows_gather_device packs, and the windows circkit_windows_of_records_device / circkit_orfs_windows_device write.
The bytes come from tests/orfs_ref.cyclic_cut (Orf::seq) and oracle.revcomp (bio's revcomp); nothing here knows a granule."""
import math

import numpy as np

from oracle import oracle as O
from tests.orfs_ref import cyclic_cut

WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])
ROTATE_BASES, ROTATE_PERCENT, CAT, DECAT, REVCOMP = range(5)
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
U64_MAX = 2 ** 64 - 1


def windows(rows):
    """[(length, record, start, strand[, reserved])] -> an array of WINDOW_DTYPE."""
    w = np.zeros(len(rows), dtype=WINDOW_DTYPE)
    for k, r in enumerate(rows):
        w[k] = tuple(r) + (0,) * (5 - len(r))
    return w


def is_invalid(w, lengths):
    r = int(w["record"])
    return r >= len(lengths) or int(w["strand"]) > 1 or int(w["reserved"]) != 0 or int(lengths[r]) >= 2 ** 32


def gather(data, offsets, wins):
    """(out_bytes, out_offsets, n_invalid): window k's bytes are out_bytes[out_offsets[k] .. out_offsets[k + 1]).  An invalid
    window and a window on an empty record write nothing."""
    raw = bytes(np.ascontiguousarray(data, dtype=np.uint8))
    offs = [int(o) for o in offsets]
    lengths = [b - a for a, b in zip(offs, offs[1:])]
    strands = {}                                          # (record, strand) -> the bytes the window reads cyclically

    def strand_of(r, s):
        if (r, s) not in strands:
            rec = raw[offs[r]:offs[r + 1]]
            strands[(r, s)] = rec if s == 0 else O.revcomp(rec)
        return strands[(r, s)]
    parts, out_off, bad = [], [0], 0
    for w in wins:
        if is_invalid(w, lengths):
            bad += 1
            cut = b""
        else:
            cut = cyclic_cut(strand_of(int(w["record"]), int(w["strand"])), int(w["start"]), int(w["length"]))
        parts.append(cut)
        out_off.append(out_off[-1] + len(cut))
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(out_off, dtype=np.uint64), bad


def as_i64(v):
    """f64 -> i64 as Rust's `as` converts: NaN is 0, the rest saturates."""
    if math.isnan(v):
        return 0
    if v >= 2.0 ** 63:
        return I64_MAX
    if v <= -2.0 ** 63:
        return I64_MIN
    return int(v)


def rotation_index(n, bases=None, percent=None):
    """src/rotate.rs:26-40 for a record of n > 0 symbols: where the rotated record starts, in 0..n (n itself included)."""
    if percent is not None:
        v = float(n) * percent
        s = as_i64(v if math.isnan(v) or math.isinf(v) else float(math.floor(v)))
    else:
        s = int(bases)
    return n - (s % n) if s >= 0 else (-s) % n


def windows_of_records(lengths, kind, bases=0, percent=0.0):
    """One window per record, by the rules of circkit_windows_of_records_device."""
    w = np.zeros(len(lengths), dtype=WINDOW_DTYPE)
    for i, n in enumerate(int(x) for x in lengths):
        length, start, strand = n, 0, 0
        if kind == CAT:
            length = min(2 * n, U64_MAX)
        elif kind == DECAT:
            length = n // 2
        elif kind == REVCOMP:
            strand = 1
        elif 0 < n < 2 ** 32:
            start = rotation_index(n, bases if kind == ROTATE_BASES else None, percent if kind == ROTATE_PERCENT else None) % n
        w[i] = (length if n else 0, i, start, strand, 0)
    return w


def orf_windows(orf_offsets, orfs, include_stop):
    """One window per ORF of an ORF batch (orfs_ref.orfs_batch's result), by the rules of circkit_orfs_windows_device."""
    counts = np.diff(np.asarray(orf_offsets, dtype=np.uint64).astype(np.int64))
    w = np.zeros(len(orfs), dtype=WINDOW_DTYPE)
    cut = 0 if include_stop else 3
    w["length"] = np.where(orfs["length"] > cut, orfs["length"] - np.uint64(cut), 0)
    w["record"] = np.repeat(np.arange(len(counts), dtype=np.uint32), counts)
    w["start"], w["strand"] = orfs["start"], orfs["strand"]
    return w
