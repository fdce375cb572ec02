"""Loads the host build of the uniq compact's decision (tests only): tests/emu/uniq_compact_emu.cpp, built like the monomer
compact's fiber library (tests/emu/compact_emu.py), with the emulator's SANITIZE flags."""
import ctypes
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "uniq_compact_emu.cpp")
_SO = os.path.join(_HERE, "libuniq_compact_emu.so")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_CSRC, "monomer_compact.h"), os.path.join(_CSRC, "wave_prims.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared"] + emu.SANITIZE + ["-o", _SO, _SRC,
                              "-L" + _HERE, "-l:libcanon_emu.so", "-Wl,-rpath,$ORIGIN"])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        ctypes.CDLL(emu.build(), mode=ctypes.RTLD_GLOBAL)
        _lib = ctypes.CDLL(build())
        _lib.emu_uniq_written_bit.restype = ctypes.c_uint64
        _lib.emu_uniq_decide.restype = None
        _lib.emu_uniq_decide.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p]
    return _lib


def decide(lengths, first_seen, base_index=0, schedule=None):
    """(kept bool[n], written length uint64[n]) as ck_compact::decide_uniq answers record by record.  The decision is per record
    and runs no fibers today; `schedule` is set round the call all the same, so that it holds the day the routine gains a collective."""
    L = lib()
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    first_seen = np.ascontiguousarray(first_seen, dtype=np.uint64)
    n = len(lengths)
    assert len(first_seen) == n
    w = np.full(n + 2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    with emu.scheduled(schedule):
        L.emu_uniq_decide(lengths.ctypes.data, first_seen.ctypes.data, int(base_index), n, w[1:].ctypes.data)
    assert w[0] == 0x5A5A5A5A5A5A5A5A and w[n + 1] == 0x5A5A5A5A5A5A5A5A
    bit = np.uint64(L.emu_uniq_written_bit())
    return (w[1:n + 1] & bit) != 0, w[1:n + 1] & ~bit
