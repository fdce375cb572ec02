"""Builds and runs the CPU fiber program of the distance unit (tests only): tests/emu/distance_emu_main.cpp, a stand-alone program
with its own main, linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE
flags (a host build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64[9] (n_a, payload bytes of A, n_b, payload bytes of B, same batch, W,
n_pairs, outputs: 1 distance | 2 scores, waves), the offsets of A (as the call gets them: the payload block starts at offset 0),
the payload of A, the same of B unless it is the same batch, the pairs.  Result: u64[3] (rc, within, invalid), the distances
(uint32 each, 0x3F bytes where nothing was written), the scores.  rc: 0, or 2 = a canary or an input changed."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "distance_emu_main.cpp")
_BIN = os.path.join(_HERE, "distance_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h")] + [os.path.join(_CSRC, f) for f in ("distance.h", "sketch.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery; nothing is preloaded
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """(DISTANCE_WAVES, SLICE_WORDS, STAGE_SLACK, DISTANCE_MAX) as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return tuple(int(v) for v in out)


def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).tobytes()


def run(cases, tmp_dir, waves=3, timeout=900, schedule=None):
    """cases: tests/distance_sets.py's Case objects.  Returns per case (distance or None, scores or None, within, invalid)."""
    blob = [_u64([len(cases)])]
    for c in cases:
        pairs = np.ascontiguousarray(np.asarray(c.pairs, dtype=np.uint64).astype(np.uint32)).reshape(-1, 2)
        want = {"both": 3, "distance": 1, "scores": 2}[c.out]
        blob += [_u64([len(c.off_a) - 1, len(c.data_a), len(c.off_b) - 1, len(c.data_b), int(c.same), c.W, len(pairs), want, waves]),
                 c.off_a.tobytes(), c.data_a.tobytes()]
        if not c.same:
            blob += [c.off_b.tobytes(), c.data_b.tobytes()]
        blob.append(pairs.tobytes())
    src, dst = os.path.join(str(tmp_dir), "distance_cases.bin"), os.path.join(str(tmp_dir), "distance_results.bin")
    with open(src, "wb") as f:
        f.write(b"".join(blob))
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "distance_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = open(dst, "rb").read()
    out, at = [], 0
    for k, c in enumerate(cases):
        m = len(c.pairs)
        rc, within, invalid = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=3, offset=at))
        at += 24
        assert rc == 0, "case %d: a canary or an input changed" % k
        dist = np.frombuffer(raw, dtype=np.uint32, count=m, offset=at).copy()
        at += 4 * m
        scores = np.frombuffer(raw, dtype=np.uint32, count=2 * m, offset=at).reshape(m, 2).copy()
        at += 8 * m
        untouched = np.uint32(0x3F3F3F3F)
        if c.out == "scores":
            assert (dist == untouched).all(), "case %d: a distance was written though none was asked for" % k
            dist = None
        if c.out == "distance":
            assert (scores == untouched).all(), "case %d: a score was written though none was asked for" % k
            scores = None
        out.append((dist, scores, within, invalid))
    assert at == len(raw)
    return out
