"""Builds and runs the CPU fiber program of the device FASTA writer (tests only): tests/emu/fasta_write_emu_main.cpp, a
stand-alone program linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE
flags (a host build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64[12] (text bytes, n_heads, n_src, flags: 1 src | 2 labels | 4 body, n_out,
body bytes, text_shift, body_shift, out_shift, capacity: 2^64 - 1 = exactly the total, alias: 0 own block | 1 in the text's | 2 in
the body's, alias_at: i64, where the output begins relative to the text / the body payload), the text, head spans[n_heads], raw
spans[n_heads] without a body, src[n_src] when flagged, labels[n_out] (WINDOW_DTYPE) when flagged, body_offsets[n_out + 1] and
the body when flagged.  Result file, per case: u64[4] (rc, total, invalid records, refused), u64 out_offsets[n_out + 1], and the
total's bytes unless the write was refused.  rc: 0, 1 = the lanes of a wave disagree on the record their search found, 2 = a
canary or an input changed.  refused: 0, 1 capacity, 2 overlap."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "fasta_write_emu_main.cpp")
_BIN = os.path.join(_HERE, "fasta_write_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")

RC = {1: "the lanes of a wave disagree on the record their search found", 2: "a canary or an input changed"}
EXACT = 2 ** 64 - 1
REFUSED_CAPACITY, REFUSED_OVERLAP = 1, 2


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h")] + \
        [os.path.join(_CSRC, f) for f in ("fasta_write.h", "monomer_compact.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """{TILE_BYTES, WRITE_WAVES, SCAN_TILE, SCAN_WG} as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return dict(zip(("TILE_BYTES", "WRITE_WAVES", "SCAN_TILE", "SCAN_WG"), (int(v) for v in out)))


def run(cases, tmp_dir, timeout=900, schedule=None):
    """cases: tests/fasta_write_sets.py Case objects.  Returns per case (text | None when refused, out_offsets, total, n_invalid,
    refused); asserts the program's own checks."""
    src, dst = os.path.join(str(tmp_dir), "fasta_write_cases.bin"), os.path.join(str(tmp_dir), "fasta_write_results.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for c in cases:
            p = c.place
            flags = (1 if c.src is not None else 0) | (2 if c.labels is not None else 0) | (4 if c.body is not None else 0)
            head = [len(c.text), len(c.head), c.n_src, flags, c.n_out, len(c.body) if c.body is not None else 0, p.get("text_shift", 0),
                    p.get("body_shift", 0), p.get("out_shift", 0), p.get("capacity", EXACT), p.get("alias", 0), p.get("alias_at", 0) % 2 ** 64]
            f.write(np.array(head, dtype=np.uint64).tobytes() + bytes(c.text) + c.head.tobytes())
            if c.body is None:
                f.write(c.raw.tobytes())
            if c.src is not None:
                f.write(c.src.tobytes())
            if c.labels is not None:
                f.write(c.labels.tobytes())
            if c.body is not None:
                f.write(c.offsets.tobytes() + c.body.tobytes())
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "fasta_write_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for k, c in enumerate(cases):
        rc, total, bad, refused = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=4, offset=at))
        at += 32
        assert rc == 0, "case %d (%s): %s" % (k, c.name, RC.get(rc, rc))
        off = np.frombuffer(raw, dtype=np.uint64, count=c.n_out + 1, offset=at).copy()
        at += 8 * (c.n_out + 1)
        got = None
        if not refused:
            got = raw[at:at + total]
            at += total
        out.append((got, off, total, bad, refused))
    assert at == len(raw)
    return out
