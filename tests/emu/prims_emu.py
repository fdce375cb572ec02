"""Builds and runs the CPU fiber program of the wave primitives' op table (tests only): tests/emu/prims_emu_main.cpp, a stand-alone
program linked against the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags (a host
build, run on the host).  It is started as a child process: a case file in, a result file out.

Case file, little endian: u64 n_cases, then per case u32[4] (op, mode, has memory, 0), 64 x IN_W u32 (the lanes' inputs) and,
with memory, MEM_BYTES bytes.  Result file, per case: nwaves x 64 x OUT_W u32, with memory nwaves x MEM_BYTES bytes (each wave's
copy afterwards), and u32 rc: bit 0 = a canary around an LDS slice or the exchange words, or the inputs, changed; bit 1 = a guard
page around the waves' global memory changed."""
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "prims_emu_main.cpp")
_BIN = os.path.join(_HERE, "prims_emu_main")
_OPS = os.path.join(os.path.dirname(_HERE), "prims", "prims_ops.h")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


def build():
    base = emu.build()
    deps = [_SRC, _OPS, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_CSRC, "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def run(hdr, inputs, mems, nwaves, out_w, mem_bytes, tmp_dir, timeout=600, schedule=None):
    """The arguments and results of tests/prims_probe.py's run(), with `nwaves` in place of the threads: hdr (n, 4) uint32 (op,
    mode, mem slot, 0: slot 0 = no memory), inputs (n, 64, IN_W) uint32, mems (slots, mem_bytes) uint8.  Returns out (n, nwaves,
    64, out_w) uint32 and the memory afterwards (slots, nwaves, mem_bytes) uint8; asserts the program's own checks."""
    src, dst = os.path.join(str(tmp_dir), "prims_cases.bin"), os.path.join(str(tmp_dir), "prims_results.bin")
    hdr = np.ascontiguousarray(hdr, dtype=np.uint32)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint32)
    mems = np.ascontiguousarray(mems, dtype=np.uint8)
    with open(src, "wb") as f:
        f.write(np.uint64(len(hdr)).tobytes())
        for h, i in zip(hdr, inputs):
            f.write(np.array([h[0], h[1], 1 if h[2] else 0, 0], dtype=np.uint32).tobytes())
            f.write(i.tobytes())
            if h[2]:
                f.write(mems[h[2]].tobytes())
    r = subprocess.run([build(), str(nwaves), src, dst], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "prims_emu_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    raw = np.fromfile(dst, dtype=np.uint8)
    out = np.zeros((len(hdr), nwaves, 64, out_w), dtype=np.uint32)
    after = np.repeat(mems[:, None, :], nwaves, axis=1)
    at, per = 0, nwaves * 64 * out_w * 4
    for k, h in enumerate(hdr):
        out[k] = raw[at:at + per].view(np.uint32).reshape(nwaves, 64, out_w)
        at += per
        if h[2]:
            after[h[2]] = raw[at:at + nwaves * mem_bytes].reshape(nwaves, mem_bytes)
            at += nwaves * mem_bytes
        rc = int(raw[at:at + 4].view(np.uint32)[0])
        at += 4
        assert rc == 0, "case %d: rc %d (1: an LDS canary or the inputs changed, 2: a guard page of the global memory changed)" % (k, rc)
    assert at == len(raw)
    return out, after
