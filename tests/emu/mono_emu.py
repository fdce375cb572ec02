"""Loads the CPU fiber build of the monomerize wave routine (tests only): tests/emu/mono_emu.cpp, linked against the
emulator library of tests/emu/emu.py for the fiber scheduler."""
import ctypes
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "mono_emu.cpp")
_SO = os.path.join(_HERE, "libmono_emu.so")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")

NONE = 0xFFFFFFFF


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_CSRC, "monomerize.h"), os.path.join(_CSRC, "wave_prims.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared"] + emu.SANITIZE + ["-o", _SO, _SRC,
                              "-L" + _HERE, "-l:libcanon_emu.so", "-Wl,-rpath,$ORIGIN"])
    return _SO


_lib = None


def monomerize_batch(data, offsets, seed_len=10, max_mismatch=None, min_identity=None, sensitive=False, base_shift=0, lead=0, schedule=None):
    """The wave routine on every record of a CSR batch: a uint32 array (NONE = None).  base_shift: misalignment of the
    payload pointer; lead: canary bytes in front of the first record.  The input is surrounded by canaries and checked to
    be unchanged; the output array has canaries round it."""
    global _lib
    if _lib is None:
        ctypes.CDLL(emu.build(), mode=ctypes.RTLD_GLOBAL)
        _lib = ctypes.CDLL(build())
        _lib.emu_monomerize_batch.restype = ctypes.c_int
        _lib.emu_monomerize_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint64, ctypes.c_double, ctypes.c_uint32, ctypes.c_void_p]
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    assert offsets[0] == 0
    offsets = offsets + np.uint64(lead)
    raw = np.full(64 + base_shift + lead + len(data) + 64, 0x4E, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64 + base_shift
    pad = raw[skew:]
    pad[lead:lead + len(data)] = data
    before = raw.copy()
    out = np.full(64 + n + 64, 0xA5A5A5A5, dtype=np.uint32)
    with emu.scheduled(schedule):
        rc = _lib.emu_monomerize_batch(pad.ctypes.data, offsets.ctypes.data, n, int(seed_len), int(min_identity is not None),
                                       int(max_mismatch or 0), float(min_identity) if min_identity is not None else 0.0,
                                       int(bool(sensitive)), out[64:].ctypes.data)
    assert rc == 0, "the lanes of a wave disagree on the result" if rc == -1 else "emulator refused the batch"
    assert np.array_equal(raw, before), "the routine wrote into its input"
    assert (out[:64] == 0xA5A5A5A5).all() and (out[64 + n:] == 0xA5A5A5A5).all(), "wrote outside the output array"
    return out[64:64 + n].copy()
