"""Plain Python restatement of the proteins of cyclic windows (TEST INFRASTRUCTURE ONLY): what circkit_windows_translate_device
packs.  The protein of a window is the plain translation of the bytes tests/windows_ref.gather cuts for it; nothing here knows
a granule, a strand or the origin of a record."""
import json
import os

import numpy as np

from tests import windows_ref

_CODES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "genetic_codes.json")
BASE = {ord("T"): 0, ord("C"): 1, ord("A"): 2, ord("G"): 3}       # the order of NCBI's genetic-code strings


def genetic_codes():
    """{table number: its 64 residues as bytes} from tests/golden/genetic_codes.json."""
    return {int(k): v.encode() for k, v in json.load(open(_CODES)).items()}


def as_bytes(v):
    return v.encode("latin-1") if isinstance(v, str) else bytes(v)


def translate(seq, aa, unknown=b"X", first_as_m=False):
    """len(seq) // 3 residues: codon t = seq[3t : 3t + 3] through the 64-entry table aa; a codon with a byte outside ACGT is
    `unknown`; with first_as_m the first residue is 'M' where the first codon is three ACGT symbols."""
    seq, aa, unknown = bytes(seq), as_bytes(aa), as_bytes(unknown)
    assert len(aa) == 64 and len(unknown) == 1
    out = bytearray()
    for t in range(len(seq) // 3):
        c = [BASE.get(b) for b in seq[3 * t:3 * t + 3]]
        if None in c:
            out += unknown
        elif t == 0 and first_as_m:
            out += b"M"
        else:
            out.append(aa[16 * c[0] + 4 * c[1] + c[2]])
    return bytes(out)


def windows_translate(data, offsets, wins, aa, unknown=b"X", first_as_m=False):
    """(aa_bytes, aa_offsets, n_invalid): translate() over the bytes windows_ref.gather writes for each window."""
    out, out_off, bad = windows_ref.gather(data, offsets, wins)
    raw = bytes(out)
    parts = [translate(raw[int(a):int(b)], aa, unknown, first_as_m) for a, b in zip(out_off[:-1], out_off[1:])]
    aa_off = np.zeros(len(parts) + 1, dtype=np.uint64)
    aa_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64) if parts else 0
    return np.frombuffer(b"".join(parts), dtype=np.uint8), aa_off, bad


def translate_packed(data, offsets, aa, unknown=b"X", first_as_m=False):
    """translate() over every sequence of a CSR batch in one numpy pass: (aa_bytes, aa_offsets).  For the large sets, where the
    loop above is the slow part; tests/test_translate_cpu.py holds the two together."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.asarray(offsets, dtype=np.uint64).astype(np.int64)
    aa, unknown = np.frombuffer(as_bytes(aa), dtype=np.uint8), as_bytes(unknown)
    assert len(aa) == 64 and len(unknown) == 1
    count = np.diff(offs) // 3
    aa_off = np.zeros(len(count) + 1, dtype=np.int64)
    aa_off[1:] = np.cumsum(count)
    total = int(aa_off[-1])
    first = np.repeat(offs[:-1] - 3 * aa_off[:-1], count) + 3 * np.arange(total, dtype=np.int64)      # each codon's first symbol
    lut = np.full(256, 255, dtype=np.uint8)
    for byte, code in BASE.items():
        lut[byte] = code
    c = lut[data[first[:, None] + np.arange(3)]].astype(np.int64) if total else np.zeros((0, 3), dtype=np.int64)
    bad = (c == 255).any(axis=1)
    out = aa[np.where(bad, 0, 16 * c[:, 0] + 4 * c[:, 1] + c[:, 2])]
    if first_as_m:
        out[aa_off[:-1][count > 0]] = ord("M")
    out[bad] = unknown[0]
    return out, aa_off.astype(np.uint64)
