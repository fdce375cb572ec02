"""Builds and runs the CPU fiber program of the prealign unit and the anchor routines (tests only): tests/emu/prealign_emu_main.cpp,
a stand-alone program with its own main, linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the
emulator's SANITIZE flags (a host build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64 kind and
  kind 0, anchors: u64[9] (n_records, payload bytes, lead, k, log2_bins, seed, short grid, long grid, want_counts), the offsets
      (from 0; the program adds the lead), the payload.  Result: u64[4] (rc, valid k-mers, unprocessed, long), the rows, the
      anchors, the counts when asked for.
  kind 1, votes: u64[6] (n_records, log2_bins, k, min_votes, n_pairs, waves), the rows, the anchors, the offsets, the pairs.
      Result: u64[3] (rc, aligned, invalid), the windows (24 bytes each, 0x3F where nothing was written), the scores.
  kind 2, labels: u64[2] (n_records, waves), the labels.  Result: u64 rc, the pairs.
rc: 0, or 2 = a canary or an input changed."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "prealign_emu_main.cpp")
_BIN = os.path.join(_HERE, "prealign_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")
WINDOW_DTYPE = np.dtype([("length", "<u8"), ("record", "<u4"), ("start", "<u4"), ("strand", "<u4"), ("reserved", "<u4")])


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h")] + [os.path.join(_CSRC, f) for f in ("prealign.h", "sketch.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery; nothing is preloaded
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """(SKETCH_SEG, SKETCH_WAVES, PREALIGN_WAVES) as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return tuple(int(v) for v in out)


def _run(blob, tmp_dir, timeout, schedule=None):
    src, dst = os.path.join(str(tmp_dir), "prealign_cases.bin"), os.path.join(str(tmp_dir), "prealign_results.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "prealign_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    return open(dst, "rb").read()


def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).tobytes()


def run_anchors(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(records, k, log2_bins, seed, lead, short_grid, long_grid, want_counts)].  Returns per case (rows, anchors, counts or
    None, (valid, unprocessed, long))."""
    blob = [_u64([len(cases)])]
    for seqs, k, lb, seed, lead, sg, lg, wc in cases:
        offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
        blob += [_u64([0, len(seqs), int(offsets[-1]), lead, k, lb, seed, sg, lg, int(bool(wc))]), offsets.tobytes(), b"".join(seqs)]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for c, (seqs, k, lb, seed, lead, sg, lg, wc) in enumerate(cases):
        rc, valid, unprocessed, n_long = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=4, offset=at))
        at += 32
        assert rc == 0, "case %d: a canary or an input changed" % c
        n, bins = len(seqs), 1 << lb
        rows = np.frombuffer(raw, dtype=np.uint64, count=n * bins, offset=at).reshape(n, bins).copy()
        at += 8 * n * bins
        anchors = np.frombuffer(raw, dtype=np.uint32, count=n * bins, offset=at).reshape(n, bins).copy()
        at += 4 * n * bins
        counts = None
        if wc:
            counts = np.frombuffer(raw, dtype=np.uint32, count=n, offset=at).copy()
            at += 4 * n
        out.append((rows, anchors, counts, (valid, unprocessed, n_long)))
    assert at == len(raw)
    return out


def run_votes(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(rows, anchors, offsets, k, min_votes, pairs, waves)].  Returns per case (windows, scores, aligned, invalid)."""
    blob = [_u64([len(cases)])]
    shaped = []
    for rows, anchors, offsets, k, mv, pairs, waves in cases:
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint32)
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint64).astype(np.uint32)).reshape(-1, 2)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        assert rows.shape == anchors.shape and len(offsets) == len(rows) + 1
        shaped.append(len(pairs))
        blob += [_u64([1, len(rows), rows.shape[1].bit_length() - 1, k, mv, len(pairs), waves]), rows.tobytes(), anchors.tobytes(), offsets.tobytes(),
                 pairs.tobytes()]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for c, m in enumerate(shaped):
        rc, aligned, invalid = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=3, offset=at))
        at += 24
        assert rc == 0, "case %d: a canary or an input changed" % c
        windows = np.frombuffer(raw, dtype=WINDOW_DTYPE, count=m, offset=at).copy()
        at += 24 * m
        scores = np.frombuffer(raw, dtype=np.uint32, count=2 * m, offset=at).reshape(m, 2).copy()
        at += 8 * m
        out.append((windows, scores, aligned, invalid))
    assert at == len(raw)
    return out


def run_labels(cases, tmp_dir, timeout=300, schedule=None):
    """cases: [(labels, waves)].  Returns per case the pairs (n, 2)."""
    blob = [_u64([len(cases)])]
    for labels, waves in cases:
        labels = np.ascontiguousarray(labels, dtype=np.uint64)
        blob += [_u64([2, len(labels), waves]), labels.tobytes()]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for c, (labels, _) in enumerate(cases):
        rc = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=at)[0])
        at += 8
        assert rc == 0, "case %d: a canary or an input changed" % c
        out.append(np.frombuffer(raw, dtype=np.uint32, count=2 * len(labels), offset=at).reshape(-1, 2).copy())
        at += 8 * len(labels)
    assert at == len(raw)
    return out
