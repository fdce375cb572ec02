"""Loads the CPU fiber emulator of the wave kernels (tests only)."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libcanon_emu.so")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


SANITIZE = ["-fsanitize=undefined,bounds", "-fno-sanitize-recover=undefined,bounds"]


def build():
    srcs = [os.path.join(_HERE, "emu.cpp"), os.path.join(_HERE, "wave_prims_emu.h")] + \
        [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(s) > os.path.getmtime(_SO) for s in srcs):
        # UBSan + bounds checks compiled in, no recovery: undefined shifts, misaligned or out-of-bounds accesses in the kernel
        # source abort the test process (sanitizers on the CPU build only -- the GPU pool offers none)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared"] + SANITIZE + ["-o", _SO, os.path.join(_HERE, "emu.cpp")])
    return _SO


# The fiber schedules of emu.cpp's run_block: SCHEDULES is the matrix the units run under besides the default "ascending".
SCHEDULES = ("descending", "lone-wave", "random:1", "random:2")


def child_env(schedule):
    """The environment of a stand-alone emulator program that runs under `schedule` (None: this process's own, unchanged)."""
    if schedule is None:
        return None
    env = dict(os.environ)
    env["CK_EMU_SCHEDULE"] = schedule
    return env


@contextlib.contextmanager
def scheduled(schedule):
    """Every run_block of the in-process emulator libraries runs under `schedule` inside the block (None: no change)."""
    if schedule is None:
        yield
        return
    lib = ctypes.CDLL(build(), mode=ctypes.RTLD_GLOBAL)
    lib.emu_set_schedule.argtypes = [ctypes.c_char_p]
    lib.emu_set_schedule(schedule.encode())
    try:
        yield
    finally:
        lib.emu_set_schedule(None)


_lib = None
last_fast_count = 0
last_rescued_count = 0
last_fused_hash_count = 0


# `staged`: canon_stream.h's k-th workgroup geometry (WPB, RPW, NBUF), k >= 1; TWO_ROW = the ROWS == 2 builds
STAGED_GEOMETRIES = {1: (16, 1, 2), 2: (8, 2, 3), 3: (4, 2, 2), 4: (8, 2, 2), 5: (2, 2, 4), 6: (1, 2, 3), 7: (4, 1, 4), 8: (8, 1, 6), 9: (4, 2, 4),
                     10: (16, 1, 2), 11: (4, 2, 2), 12: (8, 1, 3), 13: (8, 1, 2), 14: (4, 2, 2), 15: (8, 2, 2), 16: (4, 1, 2), 17: (8, 1, 2)}       # 13: the hash build's geometry for batches with N, 14 / 15: the pair build's, 16: the bytes-only N build's (round 4)
TWO_ROW = (10, 11, 12, 17)


def alpha_rule(data, offsets):
    """launch_canon's content rule (MODE_ALPHA): of up to 4096 evenly spaced records, one in 16 or more holds a byte
    outside ACGT among its first 1008."""
    n = len(offsets) - 1
    if n == 0:
        return False
    nc = min(n, 4096)
    step = n // nc
    ok = np.zeros(256, dtype=bool)
    ok[list(b"ACGT")] = True
    bad = 0
    for k in range(nc):
        a, b = int(offsets[k * step]), int(offsets[k * step + 1])
        bad += not ok[data[a:min(b, a + 1008)]].all()
    return bad > 0 and bad * 16 >= nc


def canonicalize_batch(data, offsets, slice_dw=1024, n_waves=3, want_hash=False, flags=0, staged=1, want_aux=True,
                       base_shift=0, lead=0, alpha=None, solo=True, mixed=False, hash_only=False, want_index=None, want_strand=None,
                       want_bytes=True, schedule=None):
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.emu_canonicalize_batch.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_uint64] + [ctypes.c_void_p] * 4 + \
            [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    # want_aux is the shorthand for both per-record outputs; want_index / want_strand, when given, ask for one of them alone.
    # want_bytes=False (or hash_only): no canonical bytes, whatever else is asked for -- e.g. lmsr (flags=1) with its index only
    want_index = want_aux if want_index is None else want_index
    want_strand = want_aux if want_strand is None else want_strand
    want_bytes = want_bytes and not hash_only
    if alpha is None:
        alpha = alpha_rule(data, offsets)
    # base_shift: misalignment of the payload pointer; lead: offsets[0] (canary bytes in front of the first record)
    assert offsets[0] == 0
    offsets = offsets + np.uint64(lead)
    raw = np.full(64 + base_shift + lead + len(data) + 64, 0x4E, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64 + base_shift         # payload pointer = 64-byte boundary + base_shift
    pad = raw[skew:]
    pad[lead:lead + len(data)] = data
    raw_out = np.full(len(raw), 0x3F, dtype=np.uint8)
    out = raw_out[skew:]
    # 64 spare entries behind every per-record output: nothing may be written there
    idx = np.full(n + 64, 0xFFFFFFFF, dtype=np.uint32)
    strand = np.full(n + 64, 0xFF, dtype=np.uint8)
    hs = np.full(n + 64, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ndef = ctypes.c_uint32(0)
    nfast = ctypes.c_uint32(0)
    nfused = ctypes.c_uint32(0)
    nresc = ctypes.c_uint32(0)
    # want_aux=False: no rotation index / strand outputs -- the streaming kernel's leaner builds (see launch_canon)
    # hash_only: no canonical bytes anywhere (launch_canon with d_hash and without d_out): views + the xxh3 pass over them
    inp = pad.copy()
    with scheduled(schedule):
        st = _lib.emu_canonicalize_batch(pad.ctypes.data, offsets.ctypes.data, n, out.ctypes.data if want_bytes else None,
                                         idx.ctypes.data if want_index else None, strand.ctypes.data if want_strand else None,
                                         hs.ctypes.data if want_hash else None,
                                         slice_dw, n_waves, ctypes.byref(ndef), flags, ctypes.byref(nfast), ctypes.byref(nfused), int(staged), ctypes.byref(nresc), int(bool(alpha)) | (0 if solo else 2) | (4 if mixed else 0))
    assert st >= 0, "emulator rejected the launch (unknown `staged` geometry?)"
    global last_fast_count, last_fused_hash_count, last_rescued_count
    last_rescued_count = nresc.value
    last_fast_count = nfast.value
    last_fused_hash_count = nfused.value
    assert (out[lead + len(data):] == 0x3F).all() and (raw_out[:skew + lead] == 0x3F).all(), "kernel wrote outside the batch"
    assert (idx[n:] == 0xFFFFFFFF).all() and (strand[n:] == 0xFF).all() and (hs[n:] == 0xA5A5A5A5A5A5A5A5).all(), \
        "kernel wrote a per-record output past record n - 1"
    assert np.array_equal(pad, inp), "kernel wrote into its input"
    return out[lead:lead + len(data)], idx[:n], strand[:n], hs[:n], st, ndef.value


def xxh3_64(b):
    global _lib
    if _lib is None:
        canonicalize_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    _lib.emu_xxh3_64.restype = ctypes.c_uint64
    _lib.emu_xxh3_64.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    buf = ctypes.create_string_buffer(bytes(b) + b"\0" * 16, len(b) + 16)
    return int(_lib.emu_xxh3_64(ctypes.addressof(buf), len(b)))


FOOTPRINT_PATTERN = 0xC5A7D1E3          # what an untouched LDS dword holds in tier_footprint()
FOOTPRINT_GUARD_DW = 256
S_OUT, S_IDX, S_STRAND = 0x3F, 0xFFFFFFFF, 0xFF


def tier_footprint(data, offsets, slice_dw, kind="tier", entries=None, solo=True, team4=True, flags=0, want_bytes=True, want_index=True,
                   want_strand=True, base_shift=0, schedule=None):
    """One 4-wave workgroup with its LDS pre-filled with FOOTPRINT_PATTERN and a guard region behind the four slices
    (emu_tier_footprint).  kind "tier": canon_kernel<4>'s loop and team pass over the list `entries` (record indices, flag bits
    allowed; entry i is wave i % 4's); "mixed" / "mixed_n": the mixed-length kernel's pure / N build over all records (record i is
    wave i % 4's).  Returns bytes (0x3F where nothing was written), index, strand, high_water (per wave slice: dwords from the
    slice's start to the last one that changed), guard_touched, deferred (the output segment's entries) and status."""
    global _lib
    if _lib is None:
        canonicalize_batch(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
    fn = _lib.emu_tier_footprint
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + \
        [ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    assert offsets[0] == 0
    raw = np.full(64 + base_shift + len(data) + 64, 0x4E, dtype=np.uint8)
    skew = (-raw.ctypes.data) % 64 + base_shift         # payload pointer = 64-byte boundary + base_shift
    pad = raw[skew:]
    pad[:len(data)] = data
    inp = raw.copy()
    raw_out = np.full(len(raw), S_OUT, dtype=np.uint8)
    out = raw_out[skew:]
    idx = np.full(n + 64, S_IDX, dtype=np.uint32)
    strand = np.full(n + 64, S_STRAND, dtype=np.uint8)
    ent = np.ascontiguousarray(entries if entries is not None else [], dtype=np.uint32)
    hw = np.zeros(4, dtype=np.uint32)
    guard = ctypes.c_uint32(0)
    deferred = np.zeros(max(len(ent), n) + 4, dtype=np.uint32)
    ndef = ctypes.c_uint32(0)
    with scheduled(schedule):
        st = fn(pad.ctypes.data, offsets.ctypes.data, n, ent.ctypes.data if len(ent) else None, len(ent), out.ctypes.data if want_bytes else None,
                idx.ctypes.data if want_index else None, strand.ctypes.data if want_strand else None, None, int(slice_dw),
                {"tier": 0, "mixed": 1, "mixed_n": 2}[kind], int(bool(solo)) | (2 if team4 else 0), int(flags), FOOTPRINT_PATTERN, hw.ctypes.data,
                ctypes.byref(guard), deferred.ctypes.data, ctypes.byref(ndef))
    assert st >= 0
    assert (out[len(data):] == S_OUT).all() and (raw_out[:skew] == S_OUT).all(), "kernel wrote outside the batch"
    assert (idx[n:] == S_IDX).all() and (strand[n:] == S_STRAND).all(), "kernel wrote a per-record output past record n - 1"
    assert np.array_equal(raw, inp), "kernel wrote into its input"
    return dict(bytes=out[:len(data)].copy(), index=idx[:n], strand=strand[:n], high_water=[int(x) for x in hw], guard_touched=guard.value,
                deferred=[int(x) for x in deferred[:ndef.value]], status=st)
