"""Builds and runs the device probe of the wave primitives (TEST INFRASTRUCTURE ONLY): tests/prims/prims_probe.hip, the op table
of tests/prims/prims_ops.h compiled against the gfx950 device half of circkit_amd/csrc/wave_prims.h with the product's flags.
tests/libck_prims_probe.so is git-ignored and travels to the GPU box like the product library; __graft_entry__.build() builds
it, the GPU test builds it when it is missing or stale."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "prims", "prims_probe.hip")
OPS = os.path.join(HERE, "prims", "prims_ops.h")
PRIMS = os.path.join(ROOT, "circkit_amd", "csrc", "wave_prims.h")
LIB = os.path.join(HERE, "libck_prims_probe.so")

GUARD = 4096            # canary bytes on either side of every device buffer
CANARY = 0xA5
PAGE = 4096


def build(force=False):
    deps = [SRC, OPS, PRIMS]
    if not force and os.path.exists(LIB) and all(os.path.getmtime(d) <= os.path.getmtime(LIB) for d in deps):
        return LIB
    import sys
    sys.path.insert(0, ROOT)
    from circkit_amd.build import _hipcc
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-Wno-inline-asm", "-o", LIB, SRC])
    return LIB


_lib = None


def _load():
    """after torch, so that the process has one HIP runtime"""
    global _lib
    if _lib is None:
        import torch  # noqa: F401
        _lib = ctypes.CDLL(build())
        _lib.ck_prims_probe_launch.restype = ctypes.c_int
        _lib.ck_prims_probe_launch.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return _lib


class _Guarded:
    """`nbytes` of device memory between canaries, its first byte on a 4 KiB boundary"""

    def __init__(self, torch, dev, nbytes, fill=None):
        self.torch, self.nbytes = torch, nbytes
        self.raw = torch.full((GUARD + PAGE + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=dev)
        self.at = GUARD + (-(self.raw.data_ptr() + GUARD)) % PAGE
        self.ptr = self.raw.data_ptr() + self.at
        assert self.ptr % PAGE == 0
        if fill is not None:
            self.raw[self.at:self.at + nbytes] = torch.from_numpy(np.ascontiguousarray(fill).view(np.uint8).reshape(-1)).to(dev)

    def host(self):
        return self.raw[self.at:self.at + self.nbytes].cpu().numpy()

    def intact(self):
        return bool((self.raw[:self.at] == CANARY).all()) and bool((self.raw[self.at + self.nbytes:] == CANARY).all())


def run(hdr, inputs, mems, threads, out_w, mem_bytes):
    """hdr: (n, 4) uint32 (op, mode, mem slot, 0); inputs: (n, 64, IN_W) uint32; mems: (slots, mem_bytes) uint8, slot 0 unused.
    One workgroup of `threads` per case.  Returns out (n, nwaves, 64, out_w) uint32 and the memory afterwards (slots, nwaves,
    mem_bytes) uint8; asserts that the canaries around every buffer and the headers and inputs are unchanged."""
    import torch
    lib = _load()
    dev = torch.device("cuda", 0)
    n, nw = len(hdr), threads // 64
    hdr = np.ascontiguousarray(hdr, dtype=np.uint32)
    inputs = np.ascontiguousarray(inputs, dtype=np.uint32)
    pool = np.ascontiguousarray(np.repeat(np.ascontiguousarray(mems, dtype=np.uint8)[:, None, :], nw, axis=1))
    d_hdr = _Guarded(torch, dev, hdr.nbytes, hdr)
    d_in = _Guarded(torch, dev, inputs.nbytes, inputs)
    d_pool = _Guarded(torch, dev, pool.nbytes, pool)
    d_out = _Guarded(torch, dev, n * nw * 64 * out_w * 4, np.full(n * nw * 64 * out_w, 0xEEEEEEEE, dtype=np.uint32))
    torch.cuda.synchronize()
    st = lib.ck_prims_probe_launch(d_hdr.ptr, d_in.ptr, d_out.ptr, d_pool.ptr, n, threads, torch.cuda.current_stream().cuda_stream)
    assert st == 0, "launch failed: HIP error %d" % st
    torch.cuda.synchronize()
    for name, b in (("headers", d_hdr), ("inputs", d_in), ("memory", d_pool), ("results", d_out)):
        assert b.intact(), "the probe wrote outside its %s" % name
    assert np.array_equal(d_hdr.host().view(np.uint32).reshape(hdr.shape), hdr), "the probe wrote into its headers"
    assert np.array_equal(d_in.host().view(np.uint32).reshape(inputs.shape), inputs), "the probe wrote into its inputs"
    out = d_out.host().view(np.uint32).reshape(n, nw, 64, out_w)
    return out, d_pool.host().reshape(pool.shape)
