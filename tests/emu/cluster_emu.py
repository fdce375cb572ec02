"""Builds and runs the CPU fiber program of the cluster unit (tests only): tests/emu/cluster_emu_main.cpp, a stand-alone program
linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags (a host build,
run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u64 kind and
  kind 0, candidates: u64[7] (n_records, log2_bins, n_bands, band_bins, capacity, waves of the keys kernel, waves of the count and
      write kernels), the rows.  Result: u64[2] (rc, total pairs), the keys (n_records * n_bands), the offsets (n_records + 1),
      the pair buffer (capacity pairs of two u32, 0x3F bytes where nothing was written).
  kind 1, a link: u64[6] (n_records, n_pairs, min_similarity_q16, min_filled, waves of the link kernel, waves of the init and
      flatten kernels), the pairs, the scores.  Result: u64[4] (rc, clusters, linked, invalid), the labels.
rc: 0, or 2 = a canary or an input changed, or a parent exceeded its index."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "cluster_emu_main.cpp")
_BIN = os.path.join(_HERE, "cluster_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")
UNWRITTEN = 0x3F3F3F3F


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h")] + [os.path.join(_CSRC, f) for f in ("cluster.h", "sketch.h", "ck_scan.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def constants():
    """(SCAN_WG, SCAN_ITEMS) as the program was compiled with them."""
    out = subprocess.run([build(), "--constants"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    return int(out[0]), int(out[1])


def _run(blob, tmp_dir, timeout, schedule=None):
    src, dst = os.path.join(str(tmp_dir), "cluster_cases.bin"), os.path.join(str(tmp_dir), "cluster_results.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([build(), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "cluster_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    return open(dst, "rb").read()


def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64).tobytes()


def run_candidates(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(rows (n, bins), n_bands, band_bins, capacity, keys_waves, emit_waves)].  Returns per case (keys (n, n_bands),
    offsets, pair buffer (capacity, 2) with UNWRITTEN where nothing was written, total)."""
    blob = [_u64([len(cases)])]
    for rows, n_bands, band_bins, capacity, keys_waves, emit_waves in cases:
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        blob += [_u64([0, len(rows), rows.shape[1].bit_length() - 1, n_bands, band_bins, capacity, keys_waves, emit_waves]), rows.tobytes()]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for k, (rows, n_bands, _, capacity, _, _) in enumerate(cases):
        rc, total = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=2, offset=at))
        at += 16
        assert rc == 0, "case %d: a canary or an input changed" % k
        n = len(rows)
        keys = np.frombuffer(raw, dtype=np.uint64, count=n * n_bands, offset=at).reshape(n, n_bands).copy()
        at += 8 * n * n_bands
        offsets = np.frombuffer(raw, dtype=np.uint64, count=n + 1, offset=at).copy()
        at += 8 * (n + 1)
        pairs = np.frombuffer(raw, dtype=np.uint32, count=2 * capacity, offset=at).reshape(capacity, 2).copy()
        at += 8 * capacity
        out.append((keys, offsets, pairs, total))
    assert at == len(raw)
    return out


def run_link(cases, tmp_dir, timeout=900, schedule=None):
    """cases: [(n, pairs (m, 2), scores (m, 2), (min_similarity_q16, min_filled), link_waves, flatten_waves)].  Returns per case
    (labels, clusters, linked, invalid)."""
    blob = [_u64([len(cases)])]
    for n, pairs, scores, (q16, min_filled), link_waves, flatten_waves in cases:
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        scores = np.ascontiguousarray(scores, dtype=np.uint32).reshape(-1, 2)
        assert len(pairs) == len(scores)
        blob += [_u64([1, n, len(pairs), q16, min_filled, link_waves, flatten_waves]), pairs.tobytes(), scores.tobytes()]
    raw = _run(b"".join(blob), tmp_dir, timeout, schedule)
    out, at = [], 0
    for k, case in enumerate(cases):
        rc, clusters, linked, invalid = (int(v) for v in np.frombuffer(raw, dtype=np.uint64, count=4, offset=at))
        at += 32
        assert rc == 0, "case %d: a canary or an input changed, or a parent exceeded its index" % k
        labels = np.frombuffer(raw, dtype=np.uint64, count=case[0], offset=at).copy()
        at += 8 * case[0]
        out.append((labels, clusters, linked, invalid))
    assert at == len(raw)
    return out
