"""Builds and runs the CPU fiber program of the sketch unit (tests only): tests/emu/sketch_emu_main.cpp, a stand-alone program
linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags (a host build,
run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64 kind and
  kind 0, a sketch: u64[10] (n_records, payload bytes, lead, in_shift, k, log2_bins, seed, workgroups of the short kernel,
      workgroups of the long kernel, want_counts), u64 offsets[n_records + 1] (the program adds lead), the payload.
      Result: u64[4] (rc, valid k-mers, unprocessed records, long records), the rows, the counts when wanted.
  kind 1, a compare: u64[6] (n_a, n_b, log2_bins, n_pairs, same, waves), the rows of a, the rows of b unless `same`, the pairs.
      Result: u64[2] (rc, invalid pairs), u32 (match, filled) per pair.
  kind 2, fmix64: u64 n, n words.  Result: n words.
rc: 0, or 2 = a canary changed, or an input did."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "sketch_emu_main.cpp")
_BIN = os.path.join(_HERE, "sketch_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_HERE, "lead_block.h")] + [os.path.join(_CSRC, f) for f in ("sketch.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """(SKETCH_SEG, SKETCH_WAVES) as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return int(out[0]), int(out[1])


def _run(blob, tmp_dir, timeout, schedule=None):
    src, dst = os.path.join(str(tmp_dir), "sketch_cases.bin"), os.path.join(str(tmp_dir), "sketch_results.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "sketch_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    return open(dst, "rb").read()


def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).tobytes()


def run_sketch(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(data, offsets, dict(k=, log2_bins=, seed=), dict(lead=, in_shift=, short_grid=, long_grid=, counts=))].  The
    offsets may name more bytes than `data` holds (a crafted record that must not be read).  Returns per case (rows (n, bins),
    counts | None, valid, unprocessed, n_long); asserts the program's own checks."""
    blob = [_u64([len(cases)])]
    for data, offsets, p, place in cases:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        blob += [_u64([0, len(offsets) - 1, len(data), place.get("lead", 0), place.get("in_shift", 0), p["k"], p["log2_bins"], p.get("seed", 0),
                       place.get("short_grid", 3), place.get("long_grid", 5), int(place.get("counts", True))]), offsets.tobytes(), data.tobytes()]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for k, (_, offsets, p, place) in enumerate(cases):
        rc, valid, unprocessed, n_long = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=4, offset=at))
        at += 32
        assert rc == 0, "case %d: a canary or an input changed" % k
        n, bins = len(offsets) - 1, 1 << p["log2_bins"]
        rows = np.frombuffer(raw, dtype=np.uint64, count=n * bins, offset=at).reshape(n, bins).copy()
        at += 8 * n * bins
        counts = None
        if place.get("counts", True):
            counts = np.frombuffer(raw, dtype=np.uint32, count=n, offset=at).copy()
            at += 4 * n
        out.append((rows, counts, valid, unprocessed, n_long))
    assert at == len(raw)
    return out


def run_compare(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(rows_a, rows_b | None for the same array, pairs (m, 2), waves)].  Returns per case (match, filled, n_invalid)."""
    blob = [_u64([len(cases)])]
    for a, b, pairs, waves in cases:
        a = np.ascontiguousarray(a, dtype=np.uint64)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        bins = a.shape[1]
        blob += [_u64([1, len(a), len(a) if b is None else len(b), bins.bit_length() - 1, len(pairs), int(b is None), waves]), a.tobytes()]
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.uint64)
            assert b.shape[1] == bins
            blob.append(b.tobytes())
        blob.append(pairs.tobytes())
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for k, (_, _, pairs, _) in enumerate(cases):
        rc, bad = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=2, offset=at))
        at += 16
        assert rc == 0, "case %d: a canary or an input changed" % k
        m = len(np.asarray(pairs).reshape(-1, 2))
        res = np.frombuffer(raw, dtype=np.uint32, count=2 * m, offset=at).reshape(m, 2).copy()
        at += 8 * m
        out.append((res[:, 0], res[:, 1], bad))
    assert at == len(raw)
    return out


def fmix64(words, tmp_dir):
    words = np.ascontiguousarray(words, dtype=np.uint64)
    raw = _run(_u64([1, 2, len(words)]) + words.tobytes(), tmp_dir, 120)
    return np.frombuffer(raw, dtype=np.uint64).copy()
