"""Builds and runs the CPU fiber program of the shared scan (tests only): tests/emu/scan_emu_main.cpp, a stand-alone program
linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags (a host
build, run on the host).  It is started as a child process: a case file in, a result file out.

A configuration is the (WG, ITEMS, Op) of a unit: CONFIGS below.  An element is W 64-bit words in the files (2 for the compact's
pair).  Case file, little endian: u64 n_cases, then per case u64[4] (routine, configuration, n, extra) and
  block_scan       WG elements                                   ->  WG elements (what is in front of each thread), WG totals
  sums_exclusive   n elements (the tile sums)                    ->  n elements (exclusive), WG totals (one per thread)
  tile_base        n words (the items), extra = tiles elements   ->  per tile WG elements (each thread's base) and WG * ITEMS
                   (sums that count as exclusive already)             words (each thread's items, 0 beyond n)
  composed         n words (lengths): tile sums, rounds, apply   ->  n words (where each item ends), the total
each followed by u64 rc: bit 0 = a canary around the LDS array or the sums changed, bit 1 = the threads of a workgroup
disagree on a total."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "scan_emu_main.cpp")
_BIN = os.path.join(_HERE, "scan_emu_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")

M64 = 2 ** 64 - 1
BLOCK_SCAN, SUMS_EXCLUSIVE, TILE_BASE, COMPOSED = range(4)
WRITTEN = 1 << 63                       # monomer_compact.h
ST_PASS, ST_HEADER, ST_SEQ = 0, 1, 2    # fasta_device.h


class Op:
    """An operation of ck_scan.h restated on Python integers: the yardstick is a sequential loop over these."""

    def __init__(self, name, words, identity, combine, item=lambda w: w):
        self.name, self.words, self.identity, self.combine, self.item = name, words, identity, combine, item

    def flat(self, elems):
        return [int(x) for e in elems for x in (e if self.words > 1 else (e,))]

    def elems(self, flat):
        flat = [int(x) for x in flat]
        return flat if self.words == 1 else [tuple(flat[k:k + self.words]) for k in range(0, len(flat), self.words)]


ADD = Op("add", 1, 0, lambda a, b: (a + b) & M64)
SAT = Op("sat_add", 1, 0, lambda a, b: min(a + b, M64))
PAIR = Op("pair", 2, (0, 0), lambda a, b: ((a[0] + b[0]) & M64, (a[1] + b[1]) & M64), item=lambda w: (w >> 63, w & ~WRITTEN & M64))
STATE = Op("state", 1, ST_PASS, lambda a, b: b if b else a)
# configuration -> (WG, ITEMS, Op): the units' own, in the order of scan_emu_main.cpp
CONFIGS = {0: (1024, 8, ADD), 1: (256, 8, SAT), 2: (256, 2, SAT), 3: (256, 8, PAIR), 4: (256, 1, STATE)}


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h")] + \
        [os.path.join(_CSRC, f) for f in ("ck_scan.h", "fasta_device.h", "monomer_compact.h", "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def exclusive(op, elems):
    """The sequential yardstick: (what is in front of each element, what all of them combine to)."""
    run, before = op.identity, []
    for e in elems:
        before.append(run)
        run = op.combine(run, e)
    return before, run


def run_both(cases, tmp_dir):
    """run() with the fibers as ascending and as descending threads: the same answers, returned once."""
    up, down = run(cases, tmp_dir), run(cases, tmp_dir, descending=True)
    assert up == down, "the order in which the fibers run changes the result"
    return up


def run(cases, tmp_dir, descending=False, timeout=600, schedule=None):
    """cases: [(routine, configuration, data, extra)]: data = the WG elements / the n sums / the n item words / the n lengths,
    extra = tile_base's sums (None otherwise).  descending: fiber f is thread WG - 1 - f (scan_emu_main.cpp).  Returns per case
      block_scan, sums_exclusive   (elements, totals: one per thread)
      tile_base                    [(bases, item words) per tile]
      composed                     (ends, total)
    and asserts the program's own checks."""
    src, dst = os.path.join(str(tmp_dir), "scan_cases.bin"), os.path.join(str(tmp_dir), "scan_results.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for routine, config, data, extra in cases:
            wg, items, op = CONFIGS[config]
            words = list(data) if routine in (TILE_BASE, COMPOSED) else op.flat(data)
            tail = op.flat(extra) if extra is not None else []
            f.write(np.array([routine, config, len(data), len(extra) if extra is not None else 0], dtype=np.uint64).tobytes())
            f.write(np.array(words + tail, dtype=np.uint64).tobytes())
    r = subprocess.run([build()] + (["--descending"] if descending else []) + [src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "scan_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint64)
    out, at = [], 0

    def take(count):
        nonlocal at
        v = raw[at:at + count]
        assert len(v) == count
        at += count
        return v

    for k, (routine, config, data, extra) in enumerate(cases):
        wg, items, op = CONFIGS[config]
        if routine in (BLOCK_SCAN, SUMS_EXCLUSIVE):
            got = (op.elems(take(len(data) * op.words)), op.elems(take(wg * op.words)))
        elif routine == TILE_BASE:
            got = [(op.elems(take(wg * op.words)), [int(x) for x in take(wg * items)]) for _ in range(len(extra))]
        else:
            got = ([int(x) for x in take(len(data))], int(take(1)[0]))
        rc = int(take(1)[0])
        assert rc == 0, "case %d: rc %d (1: a canary changed, 2: the threads disagree on a total)" % (k, rc)
        out.append(got)
    assert at == len(raw)
    return out
