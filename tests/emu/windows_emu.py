"""Builds and runs the CPU fiber program of the windows gather (tests only): tests/emu/windows_emu_main.cpp, a stand-alone
program linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags
(a host build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64[7] (n_records, n_windows, payload bytes, lead, in_shift, out_shift,
capacity; capacity 2^64 - 1 = exactly the total), u64 offsets[n_records + 1] (from 0; the program adds lead), the payload, the
windows (WINDOW_DTYPE).  Result file, per case: u64[4] (rc, total, invalid windows, refused), u64 out_offsets[n_windows + 1],
and the total's bytes unless the gather was refused.  rc: 0, 1 = the lanes of a wave disagree on the window their search
found, 2 = a canary changed, or the payload or the windows did."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "windows_emu_main.cpp")
_BIN = os.path.join(_HERE, "windows_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")

WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])
RC = {1: "the lanes of a wave disagree on the window their search found", 2: "a canary, the payload or the windows changed"}
EXACT = 2 ** 64 - 1


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_HERE, "lead_block.h")] + \
        [os.path.join(_CSRC, f) for f in ("window_gather.h", "monomer_compact.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """(TILE_BYTES, GATHER_WAVES) as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return int(out[0]), int(out[1])


def of_records(lengths, kind, bases=0, percent=0.0):
    """window_of_record() of window_gather.h on each length: an array of WINDOW_DTYPE."""
    bits = "%x" % int(np.array([percent], dtype=np.float64).view(np.uint64)[0])
    r = subprocess.run([build(), "--of-records", str(int(kind)), str(int(bases)), bits] + [str(int(n)) for n in lengths], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    w = np.zeros(len(lengths), dtype=WINDOW_DTYPE)
    for k, line in enumerate(r.stdout.split("\n")[:len(lengths)]):
        w[k] = tuple(int(v) for v in line.split())
    return w


def run(cases, tmp_dir, timeout=600, schedule=None):
    """cases: [(data, offsets, windows, dict(lead=, in_shift=, out_shift=, capacity=))].  Returns per case (out_bytes | None when
    refused, out_offsets, total, n_invalid); asserts the program's own checks."""
    src, dst = os.path.join(str(tmp_dir), "windows_cases.bin"), os.path.join(str(tmp_dir), "windows_results.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for data, offsets, windows, place in cases:
            data = np.ascontiguousarray(data, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            windows = np.ascontiguousarray(windows, dtype=WINDOW_DTYPE)
            assert offsets[0] == 0 and int(offsets[-1]) == len(data)
            head = [len(offsets) - 1, len(windows), len(data), place.get("lead", 0), place.get("in_shift", 0), place.get("out_shift", 0),
                    place.get("capacity", EXACT)]
            f.write(np.array(head, dtype=np.uint64).tobytes() + offsets.tobytes() + data.tobytes() + windows.tobytes())
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "windows_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for k, (_, _, windows, _) in enumerate(cases):
        rc, total, bad, refused = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=4, offset=at))
        at += 32
        assert rc == 0, "case %d: %s" % (k, RC.get(rc, rc))
        m = len(windows)
        off = np.frombuffer(raw, dtype=np.uint64, count=m + 1, offset=at).copy()
        at += 8 * (m + 1)
        got = None
        if not refused:
            got = np.frombuffer(raw, dtype=np.uint8, count=total, offset=at).copy()
            at += total
        out.append((got, off, total, bad))
    assert at == len(raw)
    return out
