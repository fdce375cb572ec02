"""Loads the CPU fiber build of the monomer compact (tests only): tests/emu/compact_emu.cpp, linked against the emulator
library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags (a host build, run on the host)."""
import ctypes
import os
import subprocess

import numpy as np

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "compact_emu.cpp")
_SO = os.path.join(_HERE, "libcompact_emu.so")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")

NONE = 0xFFFFFFFF
IN_CANARY, OUT_CANARY = 0x4E, 0x3F
OFF_CANARY, SRC_CANARY, END_CANARY = 0xA5A5A5A5A5A5A5A5, 0x5A5A5A5A5A5A5A5A, 0xC3C3C3C3


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_CSRC, "monomer_compact.h"), os.path.join(_CSRC, "wave_prims.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared"] + emu.SANITIZE + ["-o", _SO, _SRC,
                              "-L" + _HERE, "-l:libcanon_emu.so", "-Wl,-rpath,$ORIGIN"])
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        ctypes.CDLL(emu.build(), mode=ctypes.RTLD_GLOBAL)
        _lib = ctypes.CDLL(build())
        _lib.emu_compact_tile_bytes.restype = ctypes.c_uint32
        _lib.emu_compact_waves.restype = ctypes.c_uint32
        _lib.emu_monomers_compact.restype = ctypes.c_int
        _lib.emu_monomers_compact.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64] + [ctypes.c_void_p] * 2 + [ctypes.c_uint64] * 3 + \
            [ctypes.c_double, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    return _lib


HIGH_LEAD = 1 << 30


def tile_bytes():
    return int(lib().emu_compact_tile_bytes())


def waves():
    return int(lib().emu_compact_waves())


def compact(data, offsets, ends, full_len=None, in_shift=0, out_shift=0, lead=0, min_length=0, max_length=None, min_overlap=None,
            min_overlap_percent=None, keep_all=False, schedule=None):
    """decide + scan + the gather's workgroup body on a CSR batch: (out_data, out_offsets, out_src, kept_end).
    in_shift / out_shift: the payload / output pointer mod 16; lead: offsets[0] (canary bytes in front of the first record).
    Canaries surround the payload and every output; the input is checked to be unchanged.  A lead of HIGH_LEAD bytes and more
    (the leads that put a payload across byte 2^32 of its buffer) takes a lazily reserved mapping: the lead region is neither
    touched nor copied, canaries surround the payload only, and only that window is compared."""
    L = lib()
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    ends = np.ascontiguousarray(ends, dtype=np.uint32)
    n = len(offsets) - 1
    assert offsets[0] == 0 and len(ends) == n
    nb = len(data)
    offsets = offsets + np.uint64(lead)
    if lead >= HIGH_LEAD:
        import mmap
        raw = np.frombuffer(mmap.mmap(-1, 64 + in_shift + lead + nb + 64, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000)),
                            dtype=np.uint8)
    else:
        raw = np.full(64 + in_shift + lead + nb + 64, IN_CANARY, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64 + in_shift
    pad = raw[skew:]
    window = raw[skew + lead - 64:skew + lead + nb + 64] if lead >= HIGH_LEAD else raw
    window[:] = IN_CANARY
    pad[lead:lead + nb] = data
    before = window.copy()
    raw_out = np.full(64 + out_shift + nb + 64, OUT_CANARY, dtype=np.uint8)
    oskew = (-raw_out.ctypes.data) % 64 + out_shift
    out = raw_out[oskew:]
    out_off = np.full(64 + n + 1 + 64, OFF_CANARY, dtype=np.uint64)
    out_src = np.full(64 + n + 64, SRC_CANARY, dtype=np.uint64)
    kept = np.full(64 + n + 64, END_CANARY, dtype=np.uint32)
    fl = np.ascontiguousarray(full_len, dtype=np.uint64) if full_len is not None else None
    m = ctypes.c_uint64(0)
    with emu.scheduled(schedule):
        rc = L.emu_monomers_compact(pad.ctypes.data, offsets.ctypes.data, n, ends.ctypes.data, fl.ctypes.data if fl is not None else None,
                                    int(min_length), 2 ** 64 - 1 if max_length is None else int(max_length), int(min_overlap or 0),
                                    float(min_overlap_percent) if min_overlap_percent is not None else 0.0, int(min_overlap_percent is not None),
                                    int(bool(keep_all)), out.ctypes.data, out_off[64:].ctypes.data, out_src[64:].ctypes.data,
                                    kept[64:].ctypes.data, ctypes.byref(m))
    assert rc == 0, "the lanes of a wave disagree on the record their search found"
    m = m.value
    assert np.array_equal(window, before), "the compact wrote into its input"
    B = int(out_off[64 + m])
    assert (raw_out[:oskew] == OUT_CANARY).all() and (out[B:] == OUT_CANARY).all(), "wrote outside [out, out + B)"
    assert (out_off[:64] == OFF_CANARY).all() and (out_off[64 + m + 1:] == OFF_CANARY).all(), "out_offsets written beyond entry m"
    assert (out_src[:64] == SRC_CANARY).all() and (out_src[64 + m:] == SRC_CANARY).all(), "out_src written beyond entry m - 1"
    assert (kept[:64] == END_CANARY).all() and (kept[64 + n:] == END_CANARY).all(), "kept_end written outside its n entries"
    return out[:B].copy(), out_off[64:64 + m + 1].copy(), out_src[64:64 + m].copy(), kept[64:64 + n].copy()
