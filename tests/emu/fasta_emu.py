"""Builds and runs the CPU fiber program of the device FASTA parser (tests only): tests/emu/fasta_emu_main.cpp, a stand-alone
program linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags
(a host build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64[6] (text bytes, flags: 1 first_chunk | 2 final_chunk, in_shift,
out_shift, record capacity, byte capacity; a capacity of 2^64 - 1 = exactly what the text needs) and the text.  Result file,
per case: u64[5] (rc, refused, records, payload bytes, consumed), then u64 offsets[R + 1], the payload, head spans[R], raw
spans[R], where R and the payload are 0 for a refused parse.  rc: 0, 2 = a canary or the text changed.  refused: 0, 1 capacity,
2 overlap, 3 the format error."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "fasta_emu_main.cpp")
_BIN = os.path.join(_HERE, "fasta_emu_main")
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "circkit_amd", "csrc")

EXACT = 2 ** 64 - 1
REFUSED_CAPACITY, REFUSED_OVERLAP, REFUSED_FORMAT = 1, 2, 3


def build():
    base = emu.build()
    host = os.path.join(_CSRC, "fasta_host.cpp")
    deps = [_SRC, base, host, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_ROOT, "include", "circkit.h")] + \
        [os.path.join(_CSRC, f) for f in ("fasta_device.h", "fasta_host.h", "monomer_compact.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery; the host packer's file for its table
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, host, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """{TILE_BYTES, SCAN_WG, WAVES} as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return {"TILE_BYTES": int(out[0]), "SCAN_WG": int(out[1]), "WAVES": int(out[2])}


def run(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(text, first_chunk, final_chunk, dict(in_shift=, out_shift=, record_capacity=, byte_capacity=))].  Returns per case
    dict(refused, records, bytes, consumed, offsets, data, head, raw); asserts the program's own checks."""
    src, dst = os.path.join(str(tmp_dir), "fasta_cases.bin"), os.path.join(str(tmp_dir), "fasta_results.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for text, first, final, place in cases:
            head = [len(text), int(bool(first)) | 2 * int(bool(final)), place.get("in_shift", 0), place.get("out_shift", 0),
                    place.get("record_capacity", EXACT), place.get("byte_capacity", EXACT)]
            f.write(np.array(head, dtype=np.uint64).tobytes() + bytes(text))
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "fasta_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for k in range(len(cases)):
        rc, refused, records, nbytes, consumed = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=5, offset=at))
        at += 40
        assert rc == 0, "case %d: a canary or the text changed" % k
        R, B = (0, 0) if refused else (records, nbytes)
        off = np.frombuffer(raw, dtype=np.uint64, count=R + 1, offset=at).copy()
        at += 8 * (R + 1)
        data = np.frombuffer(raw, dtype=np.uint8, count=B, offset=at).copy()
        at += B
        head = np.frombuffer(raw, dtype=np.uint64, count=2 * R, offset=at).reshape(R, 2).copy()
        at += 16 * R
        spans = np.frombuffer(raw, dtype=np.uint64, count=2 * R, offset=at).reshape(R, 2).copy()
        at += 16 * R
        out.append(dict(refused=refused, records=records, bytes=nbytes, consumed=consumed, offsets=off, data=data, head=head, raw=spans))
    assert at == len(raw)
    return out
