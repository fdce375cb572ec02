"""Seeded cases for every primitive of circkit_amd/csrc/wave_prims.h, family by family, shared by the CPU test (the emulator's
implementation) and the GPU test (the device's), and what the contract of tests/prims_ref.py says each case's results are
(tests only).  A case is one wave: an operation of tests/prims/prims_ops.h (names and numbers are read from its enum), the 64 x
IN_W words the primitive is to SEE -- pack() stores the inverse of the tight surroundings' input step, so both surroundings run
the same values -- and, for the cases that touch global memory, the MEM_BYTES they start from.

OPS below mirrors the op table: which input words pass through tin, and the results restated through prims_ref."""
import os
import re

import numpy as np

from tests import prims_ref as R

U32, U64 = np.uint32, np.uint64
L = np.arange(64)
_OPS_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prims", "prims_ops.h")


def _constants():
    text = open(_OPS_H).read()
    body = text[text.index("enum Op"):]
    names = re.findall(r"\b(OP_\w+)\b", body[:body.index("OP_COUNT")])
    consts = {k: int(v, 0) for k, v in re.findall(r"\b([A-Z_0-9]+) = (0x[0-9A-Fa-f]+|\d+)u?[,;]", text)}
    return {n[3:]: k for k, n in enumerate(names)}, consts


OP, _C = _constants()
IN_W, OUT_W, LDS_DW, MEM_BYTES, XCHG_DW = (_C[k] for k in ("IN_W", "OUT_W", "LDS_DW", "MEM_BYTES", "XCHG_DW"))
LDS_FILL, TIN_XOR, TIN_ADD, TOUT_XOR, TOUT_MUL, DMA_TAIL = (_C[k] for k in ("LDS_FILL", "TIN_XOR", "TIN_ADD", "TOUT_XOR", "TOUT_MUL", "DMA_TAIL"))
SLOAD_GROUPS = (4, 8, 16)           # every StreamCfg::GROUP of canon_config.h (test_prims_cpu.py checks that)
PLAIN, TIGHT = 0, 1


class Case:
    def __init__(self, op, words, mem=None, note=""):
        """words: up to IN_W - 1 values, each a scalar (wave-uniform) or 64 per-lane values"""
        self.op, self.note, self.mem = op, note, mem
        self.inp = np.zeros((64, IN_W), dtype=U32)
        assert len(words) < IN_W
        for k, w in enumerate(words):
            self.inp[:, k] = np.asarray(w, dtype=np.uint64).astype(U32)


# ------------------------------------------------------------------------------------------------
# the op table mirrored: clamps, the LDS slice, and per operation (words through tin, results)
def in_mem(off, nbytes, align=1):
    return (np.minimum(off.astype(np.int64), MEM_BYTES - nbytes)) & ~(align - 1)


def in_lds(k, dwords, align, end=LDS_DW):
    return np.minimum(k.astype(np.int64), end - dwords) & ~(align - 1)


def _lds0(n):
    return np.broadcast_to((LDS_FILL + np.arange(LDS_DW)).astype(U32), (n, LDS_DW)).copy()


def _out(n, *words):
    """(n, 64, OUT_W) with the given (n, 64) arrays as words 0.."""
    o = np.zeros((n, 64, OUT_W), dtype=U32)
    for k, w in enumerate(words):
        o[:, :, k] = w
    return o


def _lo(v):
    return (v & U64(0xFFFFFFFF)).astype(U32)


def _hi(v):
    return (v >> U64(32)).astype(U32)


def _p64(*vs):
    return [f(v) for v in vs for f in (_lo, _hi)]


def _c64(e, k):
    return (e[..., k + 1].astype(U64) << U64(32)) | e[..., k].astype(U64)


def _dump(n, lds, *extra):
    o = np.zeros((n, 64, OUT_W), dtype=U32)
    o[:, :, :12] = lds.reshape(n, 64, 12)
    for k, w in enumerate(extra):
        o[:, :, 12 + k] = w
    return o


def _u(e, k):
    """a wave-uniform word: lane 0's"""
    return e[:, 0, k]


def _simple(tin, fn):
    return tin, lambda e, mem, nw: {"out": fn(e)}


def _row_shr(n_):
    return _simple((0,), lambda e: _out(len(e), R.dpp_row_shr(e[..., 0], n_)))


def _x_ids(e, mem, nw):
    out = np.repeat(_out(len(e), R.lane_id(e[..., 0]))[:, None], nw, axis=1)
    for w in range(nw):
        out[:, w, :, 1] = R.wave_in_block(w, e[..., 0])
    return {"out": out}


def _x_barrier(e, mem, nw):
    total = (_u(e, 0).astype(np.int64) * nw + nw * (nw - 1) // 2) & 0xFFFFFFFF
    return {"out": _out(len(e), np.broadcast_to(total[:, None], (len(e), 64)))}


def _x_load16(e, mem, nw):
    v = R.load16(mem, in_mem(e[..., 0], 16))
    return {"out": _out(len(e), *[v[..., k] for k in range(4)])}


def _x_lds_rw16(e, mem, nw):
    n = len(e)
    lds = R.lds_store16(_lds0(n), in_lds(e[..., 0], 4, 4), e[..., 1:5])
    v = R.lds_load16(lds, in_lds(e[..., 5], 4, 4))
    return {"out": _dump(n, lds, *[v[..., k] for k in range(4)])}


def _x_atomic_add(e, mem, nw):
    k = in_mem(e[..., 0], 4, 4) // 4
    words, olds = R.atomic_add_u32(np.ascontiguousarray(mem).view(U32), k, e[..., 1])
    return {"out": _out(len(e), olds), "mem": np.ascontiguousarray(words).view(np.uint8), "olds": (0, k)}


def _x_lds_atomics(e, mem, nw):
    n, q = len(e), LDS_DW // 4
    k0 = in_lds(e[..., 0], 1, 1, q)
    lds, olds = R.lds_atomic_inc(_lds0(n), k0)
    lds = R.lds_atomic_or(lds, q + in_lds(e[..., 1], 1, 1, q), e[..., 2])
    lds = R.lds_atomic_min(lds, 2 * q + in_lds(e[..., 3], 1, 1, q), e[..., 4])
    lds = R.lds_atomic_add(lds, 3 * q + in_lds(e[..., 5], 1, 1, q), e[..., 6])
    return {"out": _dump(n, lds, olds), "olds": (12, k0)}


def _x_sload_group(span):
    def fn(e, mem, nw):
        p, q = in_mem(_u(e, 0), 8 * span + 8, 8), in_mem(_u(e, 1), 24, 8)
        vs = R.sload_group(mem, p, q, span)
        return {"out": _out(len(e), *[np.broadcast_to(w[:, None], (len(e), 64)) for w in _p64(*vs)])}
    return (), fn


def _bc(n, *vs):
    return _out(n, *[np.broadcast_to(w[:, None], (n, 64)) for w in _p64(*vs)])


def _x_glds16(e, mem, nw):
    n = len(e)
    lds = R.glds16_async(_lds0(n), in_lds(_u(e, 1), 256, 4, DMA_TAIL), mem, in_mem(e[..., 0], 16))
    lds[:, DMA_TAIL:DMA_TAIL + 64] = e[..., 3]
    return {"out": _dump(n, lds, e[..., 3][:, L ^ 1])}


def _x_glds16_s(e, mem, nw):
    n = len(e)
    return {"out": _dump(n, R.glds16_async_s(_lds0(n), in_lds(_u(e, 1), 256, 4), mem, in_mem(e[..., 0], 16)))}


def _x_glds16_s_two(e, mem, nw):
    n = len(e)
    first = in_lds(_u(e, 1), 512, 4)
    lds = R.glds16_async_s(_lds0(n), first, mem, in_mem(e[..., 0], 16))
    v = R.lds_load16(lds, first[:, None] + 4 * L)           # behind vmem_wait<1>: the first image is complete
    lds = R.glds16_async_s(lds, first + 256, mem, in_mem(e[..., 2], 16))
    return {"out": _dump(n, lds, *[v[..., k] for k in range(4)])}


def _x_glds4_touch(e, mem, nw):
    n = len(e)
    return {"out": _dump(n, R.glds4_touch(_lds0(n), in_lds(_u(e, 1), 64, 4), mem, in_mem(e[..., 0], 4)))}


def _nz32(v):
    return np.where(v == 0, U32(1), v)


def _nz64(v):
    return np.where(v == 0, U64(1), v)


OPS = {
    "IDS": ((), _x_ids),
    "BARRIER": ((0,), _x_barrier),
    "WAVE_MIN": _simple((0,), lambda e: _out(len(e), R.wave_min_u32(e[..., 0]))),
    "ROW_MIN16": _simple((0,), lambda e: _out(len(e), R.row_min16_u32(e[..., 0]))),
    "WAVE_MIN2": _simple((0, 1), lambda e: _out(len(e), *R.wave_min2_u32(e[..., 0], e[..., 1]))),
    "HALF_MIN2": _simple((0, 1), lambda e: _out(len(e), *R.half_min2_u32(e[..., 0], e[..., 1]))),
    "HALF_MIN2_BCAST": _simple((0, 1), lambda e: _out(len(e), *R.half_min2_bcast_u32(e[..., 0], e[..., 1]))),
    "PK_MIN_U16": _simple((0, 1), lambda e: _out(len(e), R.pk_min_u16(e[..., 0], e[..., 1]))),
    "ROWSUM4": _simple((0, 1, 2, 3), lambda e: _out(len(e), *_p64(*R.dpp_rowsum4_u64x2(_c64(e, 0), _c64(e, 2))))),
    "QUADSUM": _simple((0, 1), lambda e: _out(len(e), *_p64(R.dpp_quadsum_u64(_c64(e, 0))))),
    "WAVE_SUM": _simple((0, 1), lambda e: _out(len(e), *_p64(R.wave_sum_u64(_c64(e, 0))))),
    "ADD64_PARTS": _simple((0, 1, 2, 3), lambda e: _out(len(e), *_p64(R.add64_parts(_c64(e, 0), e[..., 2], e[..., 3])))),
    "MULHI64": _simple((0, 1, 2, 3), lambda e: _out(len(e), *_p64(R.mulhi64(_c64(e, 0), _c64(e, 2))))),
    "SHFL": _simple((0, 1), lambda e: _out(len(e), R.shfl(e[..., 0], e[..., 1]))),
    "READLANE": _simple((0,), lambda e: _out(len(e), R.readlane(e[..., 0], e[..., 1]))),
    "UNIFORM": _simple((0,), lambda e: _out(len(e), R.uniform(e[..., 0]))),
    "UNIFORM64": _simple((0, 1), lambda e: _out(len(e), *_p64(R.uniform64(_c64(e, 0))))),
    "WAVE_SHL1": _simple((0,), lambda e: _out(len(e), R.wave_shl1(e[..., 0]))),
    "QUAD_XOR1": _simple((0,), lambda e: _out(len(e), R.dpp_quad_xor1(e[..., 0]))),
    "QUAD_XOR2": _simple((0,), lambda e: _out(len(e), R.dpp_quad_xor2(e[..., 0]))),
    "HALF_BCAST": _simple((0,), lambda e: _out(len(e), *R.half_bcast(e[..., 0]))),
    "BALLOT": _simple((0,), lambda e: _out(len(e), *_p64(R.ballot(e[..., 0] & U32(1))))),
    "LANE_PRED": _simple((), lambda e: _out(len(e), R.lane_pred(_c64(e, 0)[:, 0], e[..., 0]).astype(U32))),
    "FUNNEL": _simple((0, 1, 2), lambda e: _out(len(e), R.funnel(e[..., 0], e[..., 1], e[..., 2] & U32(31)))),
    "ALIGNBIT": _simple((0, 1, 2), lambda e: _out(len(e), R.alignbit(e[..., 0], e[..., 1], e[..., 2]))),
    "LSHR64": _simple((0, 1, 2), lambda e: _out(len(e), R.lshr64(e[..., 0], e[..., 1], e[..., 2] & U32(63)))),
    "BFI": _simple((0, 1, 2), lambda e: _out(len(e), R.bfi(e[..., 0], e[..., 1], e[..., 2]))),
    "BFI_V": _simple((0, 1, 2), lambda e: _out(len(e), R.bfi_v(e[..., 0], e[..., 1], e[..., 2]))),
    "PERM": _simple((0, 1, 2), lambda e: _out(len(e), R.perm(e[..., 0], e[..., 1], e[..., 2]))),
    "BITREV": _simple((0,), lambda e: _out(len(e), R.bitrev(e[..., 0]))),
    "FFS32": _simple((0,), lambda e: _out(len(e), R.ffs32(_nz32(e[..., 0])))),
    "FFS64": _simple((0, 1), lambda e: _out(len(e), R.ffs64(_nz64(_c64(e, 0))))),
    "CLZ32": _simple((0,), lambda e: _out(len(e), R.clz32(_nz32(e[..., 0])))),
    "POPC32": _simple((0,), lambda e: _out(len(e), R.popc32(e[..., 0]))),
    "POPC64": _simple((0, 1), lambda e: _out(len(e), R.popc64(_c64(e, 0)))),
    "FFS32_OR_NEG": _simple((), lambda e: _out(len(e), R.ffs32_or_neg(R.uniform(e[..., 0])))),
    "FFS64_OR_NEG": _simple((0, 1), lambda e: _out(len(e), R.ffs64_or_neg(_c64(e, 0)))),
    "LOW_MASK16": _simple((), lambda e: _out(len(e), R.low_mask16(R.uniform(e[..., 0])))),
    "SAD_U8": _simple((0, 1, 2), lambda e: _out(len(e), R.sad_u8(e[..., 0], e[..., 1], e[..., 2]))),
    "UDOT4": _simple((0, 1, 2), lambda e: _out(len(e), R.udot4(e[..., 0], e[..., 1], e[..., 2]))),
    "LOAD16": ((), _x_load16),
    "LOAD4": ((), lambda e, mem, nw: {"out": _out(len(e), R.load4(mem, in_mem(e[..., 0], 4)))}),
    "STORE16": ((1, 2, 3, 4), lambda e, mem, nw: {"out": _out(len(e)), "mem": R.store16(mem, in_mem(e[..., 0], 16), e[..., 1:5])}),
    "STORE8": ((1, 2), lambda e, mem, nw: {"out": _out(len(e)), "mem": R.store8(mem, in_mem(e[..., 0], 8), e[..., 1], e[..., 2])}),
    "STORE4": ((1,), lambda e, mem, nw: {"out": _out(len(e)), "mem": R.store4(mem, in_mem(e[..., 0], 4), e[..., 1])}),
    "LDS_RW16": ((1, 2, 3, 4), _x_lds_rw16),
    "ATOMIC_ADD": ((1,), _x_atomic_add),
    "LDS_ATOMICS": ((2, 4, 6), _x_lds_atomics),
    "SLOAD_U64X2": ((), lambda e, mem, nw: {"out": _bc(len(e), *R.sload_u64x2(mem, in_mem(_u(e, 0), 16, 8)))}),
    "SLOAD_2U64": ((), lambda e, mem, nw: {"out": _bc(len(e), *R.sload_2u64(mem, in_mem(_u(e, 0), 8, 8), in_mem(_u(e, 1), 8, 8)))}),
    "GLDS16": ((3,), _x_glds16),
    "GLDS16_S": ((), _x_glds16_s),
    "GLDS16_S_TWO": ((), _x_glds16_s_two),
    "GLDS4_TOUCH": ((), _x_glds4_touch),
}
for _n in range(1, 16):
    OPS["ROW_SHR_%d" % _n] = _row_shr(_n)
for _g in SLOAD_GROUPS:
    OPS["SLOAD_GROUP_%d" % _g] = _x_sload_group(_g)
# which primitive of the interface each operation is there for (test_prims_cpu.py: every primitive has one)
PRIMITIVES = {
    "IDS": ("lane_id", "wave_in_block"), "BARRIER": ("block_barrier",), "WAVE_MIN": ("wave_min_u32",), "ROW_MIN16": ("row_min16_u32",),
    "WAVE_MIN2": ("wave_min2_u32",), "HALF_MIN2": ("half_min2_u32",), "HALF_MIN2_BCAST": ("half_min2_bcast_u32",), "PK_MIN_U16": ("pk_min_u16",),
    "ROWSUM4": ("dpp_rowsum4_u64x2",), "QUADSUM": ("dpp_quadsum_u64",), "WAVE_SUM": ("wave_sum_u64",), "ADD64_PARTS": ("add64_parts",),
    "MULHI64": ("mulhi64",), "SHFL": ("shfl",), "READLANE": ("readlane", "uniform"), "UNIFORM": ("uniform",), "UNIFORM64": ("uniform64",),
    "WAVE_SHL1": ("wave_shl1",), "QUAD_XOR1": ("dpp_quad_xor1",), "QUAD_XOR2": ("dpp_quad_xor2",), "HALF_BCAST": ("half_bcast",),
    "BALLOT": ("ballot",), "LANE_PRED": ("lane_pred", "uniform64"), "FUNNEL": ("funnel",), "ALIGNBIT": ("alignbit",), "LSHR64": ("lshr64",),
    "BFI": ("bfi",), "BFI_V": ("bfi_v",), "PERM": ("perm",), "BITREV": ("bitrev",), "FFS32": ("ffs32",), "FFS64": ("ffs64",), "CLZ32": ("clz32",),
    "POPC32": ("popc32",), "POPC64": ("popc64",), "FFS32_OR_NEG": ("ffs32_or_neg",), "FFS64_OR_NEG": ("ffs64_or_neg",),
    "LOW_MASK16": ("low_mask16",), "SAD_U8": ("sad_u8",), "UDOT4": ("udot4",), "LOAD16": ("load16",), "LOAD4": ("load4",),
    "STORE16": ("store16",), "STORE8": ("store8",), "STORE4": ("store4",), "LDS_RW16": ("lds_store16", "lds_load16", "wave_sync"),
    "ATOMIC_ADD": ("atomic_add_u32",), "LDS_ATOMICS": ("lds_atomic_inc", "lds_atomic_or", "lds_atomic_min", "lds_atomic_add"),
    "SLOAD_U64X2": ("sload_u64x2",), "SLOAD_2U64": ("sload_2u64",), "GLDS16": ("glds16_async", "vmem_wait"), "GLDS16_S": ("glds16_async_s",),
    "GLDS16_S_TWO": ("glds16_async_s", "vmem_wait"), "GLDS4_TOUCH": ("glds4_touch",),
}
for _n in range(1, 16):
    PRIMITIVES["ROW_SHR_%d" % _n] = ("dpp_row_shr",)
for _g in SLOAD_GROUPS:
    PRIMITIVES["SLOAD_GROUP_%d" % _g] = ("sload_group",)


# ------------------------------------------------------------------------------------------------
# the cases
def _rng(name):
    return np.random.default_rng([0x9F1A, sum(name.encode())])


def _r32(rng, lo=0, hi=0xFFFFFFFF):
    return rng.integers(lo, hi, size=64, dtype=np.uint64, endpoint=True)


def _mem(rng):
    return rng.integers(0, 256, size=MEM_BYTES, dtype=np.uint8)


def minima():
    rng, cases = _rng("minima"), []
    regimes = ((0x10, 0xFFFFFFFF), (0x7FFFFFFF, 0x80000010), (0x80000000, 0xFFFFFFFF), (0, 0x7FFFFFFF))
    ops = ("WAVE_MIN", "ROW_MIN16", "WAVE_MIN2", "HALF_MIN2", "HALF_MIN2_BCAST")

    def both(x, y, note):
        for op in ops:
            cases.append(Case(op, (x, y), note=note))

    for k in range(64):                                     # the unique minimum in every lane in turn; y's in another row
        (lo, hi), (lo2, hi2) = regimes[k % 4], regimes[(k // 4 + 1) % 4]
        x, y = _r32(rng, lo + 1, hi), _r32(rng, lo2 + 1, hi2)
        ky = ((k + 16 * (1 + k % 3)) % 64) ^ 5
        assert ky // 16 != k // 16
        x[k], y[ky] = lo, lo2
        both(x, y, "unique minimum: x lane %d, y lane %d" % (k, ky))
    for a, b in ((15, 16), (31, 32), (47, 48)):             # ties across the row boundaries
        x, y = _r32(rng, 0x80000001, 0xFFFFFFFF), _r32(rng, 6, 0xFFFFFFFF)
        x[[a, b]] = 0x80000000
        y[[b, a]] = 5
        both(x, y, "tie across %d/%d" % (a, b))
    for c in (0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, int(rng.integers(1, 2 ** 32 - 1))):
        both(np.full(64, c, dtype=np.uint64), np.full(64, c ^ 0x80000000, dtype=np.uint64), "all equal %#x" % c)
    x = np.where(L < 32, 0xFFFFFFFF, 0).astype(np.uint64)   # each half its own extreme
    both(x, x[::-1].copy(), "halves 0xFFFFFFFF / 0")
    # pk_min_u16: per lane, both halves on both sides of 0x8000
    edge = np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFE, 0xFFFF, 0x1234], dtype=np.uint64)
    a = (edge[L % 8] << np.uint64(16)) | edge[(L // 8) % 8]
    b = (edge[(L // 8) % 8] << np.uint64(16)) | edge[L % 8]
    cases.append(Case("PK_MIN_U16", (a, b), note="edges"))
    cases.append(Case("PK_MIN_U16", (b, a[::-1].copy()), note="edges, crossed"))
    for _ in range(3):
        cases.append(Case("PK_MIN_U16", (_r32(rng), _r32(rng)), note="random"))
    return cases


def sums():
    rng, cases = _rng("sums"), []
    ones = np.full(64, 0xFFFFFFFF, dtype=np.uint64)
    zero = np.zeros(64, dtype=np.uint64)
    pats = [((ones, _r32(rng, 0, 0xFFFF), ones, _r32(rng, 0, 0xFFFF)), "low words 0xFFFFFFFF: every step carries"),
            ((zero, _r32(rng), zero, _r32(rng)), "high word only"),
            ((ones, _r32(rng), zero + 1, _r32(rng)), "a carries, b does not"),
            ((zero + 1, _r32(rng), ones, _r32(rng)), "b carries, a does not"),
            ((ones, ones, ones, ones), "all ones: wraps past 2^64"),
            ((ones, zero, zero + 1, zero), "0xFFFFFFFF + 1 chains"),
            ((_r32(rng, 0x80000000, 0xFFFFFFFF), zero, _r32(rng, 0x80000000, 0xFFFFFFFF), ones), "top bits of the low words")]
    for _ in range(4):
        pats.append(((_r32(rng), _r32(rng), _r32(rng), _r32(rng)), "random"))
    for k in (0, 3, 4, 11, 12, 15, 16, 35, 63):             # one lane's carry, seen by the lanes behind it
        al, bl = zero + 1, zero + 2
        al[k], bl[63 - k] = 0xFFFFFFFF, 0xFFFFFFFE
        pats.append(((al, (L * 3).astype(np.uint64), bl, (L * 5 + 1).astype(np.uint64)), "carry out of lane %d" % k))
    for words, note in pats:
        for op in ("ROWSUM4", "QUADSUM", "WAVE_SUM", "ADD64_PARTS", "MULHI64"):
            cases.append(Case(op, words, note=note))
    # mulhi64 / add64_parts: extremes per lane
    ext = np.array([0, 1, 2, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x10000, 0xFFFF], dtype=np.uint64)
    for op in ("MULHI64", "ADD64_PARTS"):
        cases.append(Case(op, (ext[L % 8], ext[(L // 8) % 8], ext[(L // 8) % 8], ext[(7 - L % 8)]), note="extremes"))
    return cases


def lane_moves():
    rng, cases = _rng("lane_moves"), []
    special = [64, 65, 127, 255, 256, 257, 256 + 63, 0x40000000, 0xFFFFFFFF, 0xFFFFFFC0, 0x80000001]
    for s in list(range(64)) + special:                     # wave-uniform sources
        cases.append(Case("SHFL", (_r32(rng), s), note="uniform source %#x" % s))
    per_lane = [((L + 1), "lane + 1 (64 in lane 63)"), ((L.astype(np.int64) - 5) & 0xFFFFFFFF, "lane - 5 (wraps below 0)"),
                (63 - L, "reversed"), (_r32(rng, 0, 63), "random lanes"), (_r32(rng), "random words"),
                (np.array(special, dtype=np.uint64)[L % len(special)], "the special sources"), (256 + L[::-1], "256 + k"), (L ^ 32, "other half")]
    for src, note in per_lane:
        cases.append(Case("SHFL", (_r32(rng), np.asarray(src, dtype=np.uint64)), note=note))
    for lane in range(64):
        cases.append(Case("READLANE", (_r32(rng), lane), note="lane %d" % lane))
    full = np.full(64, 0xFFFFFFFF, dtype=np.uint64)
    one_var = ["UNIFORM", "WAVE_SHL1", "QUAD_XOR1", "QUAD_XOR2", "HALF_BCAST"] + ["ROW_SHR_%d" % n for n in range(1, 16)]
    for op in one_var:
        cases.append(Case(op, (_r32(rng),), note="random"))
        cases.append(Case(op, (_r32(rng, 1, 0xFFFFFFFF),), note="random, no zero"))
        cases.append(Case(op, (full,), note="all ones"))
    for _ in range(3):
        cases.append(Case("UNIFORM64", (_r32(rng), _r32(rng)), note="random"))
    masks = [0, 2 ** 64 - 1, 0xFFFFFFFF, 0xFFFFFFFF00000000] + [1 << k for k in (0, 1, 15, 16, 31, 32, 47, 48, 62, 63)] + \
        [int(rng.integers(0, 2 ** 64, dtype=np.uint64)) for _ in range(3)]
    for m in masks:
        bits = np.array([(m >> k) & 1 for k in range(64)], dtype=np.uint64)
        cases.append(Case("BALLOT", ((_r32(rng) & np.uint64(0xFFFFFFFE)) | bits,), note="mask %#x" % m))
        cases.append(Case("LANE_PRED", (m & 0xFFFFFFFF, m >> 32), note="mask %#x" % m))
    cases.append(Case("IDS", (), note="lane_id, wave_in_block"))
    for c in (0, 0xFFFFFFF0, int(rng.integers(0, 2 ** 32))):
        cases.append(Case("BARRIER", (c,), note="exchange across the barrier, %#x" % c))
    return cases


PERM_ALLOWED = list(range(8)) + list(range(12, 256))        # selector bytes inside the contract


def words():
    rng, cases = _rng("words"), []
    ones = np.full(64, 0xFFFFFFFF, dtype=np.uint64)
    for sh in range(32):
        cases.append(Case("FUNNEL", (_r32(rng), _r32(rng), sh), note="uniform sh %d" % sh))
    for s in range(64):
        cases.append(Case("ALIGNBIT", (_r32(rng), _r32(rng), s), note="uniform s %d" % s))
        cases.append(Case("LSHR64", (_r32(rng), _r32(rng), s), note="uniform s %d" % s))
    for op, m in (("FUNNEL", 31), ("ALIGNBIT", 63), ("LSHR64", 63)):
        cases.append(Case(op, (_r32(rng), _r32(rng), L & m), note="s = lane"))
        cases.append(Case(op, (ones, np.zeros(64), (63 - L) & m), note="s = 63 - lane, ones:zeros"))
        cases.append(Case(op, (np.zeros(64), ones, _r32(rng, 0, m)), note="random s, zeros:ones"))
    cases.append(Case("ALIGNBIT", (_r32(rng), _r32(rng), _r32(rng)), note="any s: only s mod 32 counts"))
    single = np.uint64(1) << (L % 32).astype(np.uint64)
    for op in ("BFI", "BFI_V"):
        cases.append(Case(op, (_r32(rng), _r32(rng), _r32(rng)), note="random"))
        cases.append(Case(op, (single, ones, np.zeros(64)), note="single-bit masks"))
        cases.append(Case(op, (np.where(L & 1, 0xFFFFFFFF, 0), _r32(rng), _r32(rng)), note="full and empty masks"))
    allowed = np.array(PERM_ALLOWED, dtype=np.uint64)
    for k in range(0, len(allowed), 64):                    # every selector byte of the contract, in all four positions
        sel = allowed[(k + L) % len(allowed)] * np.uint64(0x01010101)
        cases.append(Case("PERM", (_r32(rng), _r32(rng), sel), note="selector bytes from %#x" % int(allowed[k])))
    for _ in range(4):
        sel = sum(allowed[rng.integers(0, len(allowed), 64)] << np.uint64(8 * i) for i in range(4))
        cases.append(Case("PERM", (_r32(rng), _r32(rng), sel), note="mixed selectors"))
    for sel in (0x00010203, 0x04050607, 0x0c0c0c00, 0x07060504, 0x0c020c00, 0xff0d0c03):
        cases.append(Case("PERM", (_r32(rng), _r32(rng), sel), note="uniform selector %#x" % sel))
    bit64 = np.uint64(1) << L.astype(np.uint64)
    for op in ("BITREV", "FFS32", "CLZ32", "POPC32"):
        for v, note in ((single, "single bits"), (ones, "all ones"), (_r32(rng), "random"), (ones << (L % 32).astype(np.uint64), "runs of ones from bit k"),
                        (ones >> (L % 32).astype(np.uint64), "runs of ones below bit k")):
            cases.append(Case(op, (v & np.uint64(0xFFFFFFFF),), note=note))
    cases.append(Case("POPC32", (np.zeros(64),), note="0"))
    for op in ("FFS64", "POPC64", "FFS64_OR_NEG"):
        for v, note in ((bit64, "single bits"), (np.full(64, 2 ** 64 - 1, dtype=np.uint64), "all ones"),
                        ((_r32(rng) << np.uint64(32)) | _r32(rng), "random"), (_r32(rng) << np.uint64(32), "high word only"),
                        (np.full(64, 2 ** 64 - 1, dtype=np.uint64) << L.astype(np.uint64), "runs of ones from bit k")):
            cases.append(Case(op, (v & np.uint64(0xFFFFFFFF), v >> np.uint64(32)), note=note))
    cases.append(Case("FFS64_OR_NEG", (np.where(L & 1, 0, 8), np.zeros(64)), note="0 gives -1"))
    cases.append(Case("POPC64", (np.zeros(64), np.zeros(64)), note="0"))
    for v in [0, 0xFFFFFFFF, 0x80000000, 0xFFFF0000] + [1 << k for k in range(0, 32, 3)] + [int(x) for x in rng.integers(0, 2 ** 32, 4)]:
        cases.append(Case("FFS32_OR_NEG", (v,), note="%#x" % v))
    for v in (0, 1, 2, 7, 15, 16, 17, 31, 32, 33, 2 ** 31, 2 ** 32 - 1):
        cases.append(Case("LOW_MASK16", (v,), note="left %#x" % v))
    cases.append(Case("SAD_U8", (np.zeros(64), ones, (2 ** 32 - 1020 + L * 16) % 2 ** 32), note="0 against 0xFF bytes, acc wraps"))
    cases.append(Case("SAD_U8", (ones, np.zeros(64), _r32(rng)), note="0xFF bytes against 0"))
    for _ in range(3):
        cases.append(Case("SAD_U8", (_r32(rng), _r32(rng), _r32(rng)), note="random"))
    top = 255 * 255 * 4
    cases.append(Case("UDOT4", (ones, ones, (2 ** 32 - top - 32 + L) % 2 ** 32), note="255 * 255 * 4 + c across 2^32"))
    cases.append(Case("UDOT4", (ones, ones, L * 0x04000000), note="255 * 255 * 4 + c"))
    for _ in range(3):
        cases.append(Case("UDOT4", (_r32(rng), _r32(rng), _r32(rng)), note="random"))
    return cases


def access():
    rng, cases = _rng("access"), []
    width = {"LOAD16": 16, "LOAD4": 4, "STORE16": 16, "STORE8": 8, "STORE4": 4}
    for op, wd in width.items():
        for shift in range(16):                             # every byte shift of the base; the lanes' ranges are disjoint
            order = rng.permutation(64) if shift & 1 else L
            cases.append(Case(op, (256 + shift + 32 * order, _r32(rng), _r32(rng), _r32(rng), _r32(rng)), mem=_mem(rng), note="shift %d" % shift))
        # lane 31's bytes straddle byte 4096 of the case's memory (which begins on a 4 KiB boundary)
        cases.append(Case(op, (4096 - wd // 2 - 32 * 31 + 32 * L, _r32(rng), _r32(rng), _r32(rng), _r32(rng)), mem=_mem(rng), note="astride 4 KiB"))
        cases.append(Case(op, (np.where(L == 0, 0, np.where(L == 63, MEM_BYTES - wd, 512 + 17 * L))[rng.permutation(64)], _r32(rng), _r32(rng), _r32(rng),
                               _r32(rng)), mem=_mem(rng), note="first and last bytes"))
    for base in (0, 4, 256, 508, 512):
        st, ld = 4 * rng.permutation(64) + base, 4 * rng.permutation(64) + base
        cases.append(Case("LDS_RW16", (st, _r32(rng), _r32(rng), _r32(rng), _r32(rng), ld), note="16-byte slots from dword %d" % base))
    cases.append(Case("LDS_RW16", (12 * L, _r32(rng), _r32(rng), _r32(rng), _r32(rng), 12 * (63 - L) + 8), note="strided"))
    return cases


def atomics():
    rng, cases = _rng("atomics"), []
    for off, v, note in ((64, 3, "one word"), (4096 - 4, 0x11111111, "one word below 4 KiB, wraps"), (8188, 0xFFFFFFFF, "the last word, adds -1"),
                         (128 + 4 * rng.permutation(64), _r32(rng), "64 words"), (1024 + 4 * (L % 4), 1 + (L % 4) * 0x01000000, "four words"),
                         (4 * (L // 32) + 4092, 7, "a word either side of 4 KiB")):
        cases.append(Case("ATOMIC_ADD", (off, v), mem=_mem(rng), note=note))
    q = LDS_DW // 4
    sets = [(np.zeros(64), "one word"), (rng.permutation(64) + 5, "64 words"), (L % 4 + q - 4, "four words"), (L // 32 * (q - 1), "first and last")]
    for k, note in sets:
        cases.append(Case("LDS_ATOMICS", (k, k, np.uint64(1) << (L % 32).astype(np.uint64), k, _r32(rng), k, np.full(64, 0x10000001)), note=note))
        cases.append(Case("LDS_ATOMICS", (k[::-1].copy(), k, _r32(rng), k, _r32(rng, 0xC0DE0000, 0xC0DE0400), k[::-1].copy(), _r32(rng)), note=note + ", random"))
    return cases


def scalar_loads():
    rng, cases = _rng("scalar_loads"), []
    for p in (0, 8, 16, 24, 48, 56, 120, 4080, 4088, 4096, 4104, MEM_BYTES - 16):
        cases.append(Case("SLOAD_U64X2", (p,), mem=_mem(rng), note="p = %d (%d mod 16)" % (p, p % 16)))
    for p0, p1 in ((0, 8), (8, 0), (56, 64), (4088, 4096), (4096, 4088), (MEM_BYTES - 8, 0), (24, 24), (1000, 7000)):
        cases.append(Case("SLOAD_2U64", (p0, p1), mem=_mem(rng), note="p0 = %d, p1 = %d" % (p0, p1)))
    for g in SLOAD_GROUPS:
        ps = (0, 8, 64 - 8 * g + 64, 4096 - 8 * g, 4096 - 8, 4088 - 8 * g, MEM_BYTES - 8 * g - 8)
        qs = (0, 8, 48, 4080, 4088, 4072, MEM_BYTES - 24)
        for k, p in enumerate(ps):
            for q in (qs[k], qs[(k + 3) % len(qs)]):
                cases.append(Case("SLOAD_GROUP_%d" % g, (p, q), mem=_mem(rng), note="p = %d, q = %d" % (p, q)))
    return cases


def lds_dma():
    rng, cases = _rng("lds_dma"), []
    dsts = (0, 4, 64, 100, 252, 448, 8, 300)
    for op in ("GLDS16", "GLDS16_S"):
        for shift in range(16):
            order = rng.permutation(64) if shift & 1 else L
            cases.append(Case(op, (128 + shift + 32 * order, dsts[shift % len(dsts)], 0, _r32(rng)), mem=_mem(rng),
                              note="source shift %d, image at dword %d" % (shift, dsts[shift % len(dsts)])))
        cases.append(Case(op, (4096 - 8 - 16 * 31 + 16 * L, 16, 0, _r32(rng)), mem=_mem(rng), note="lane 31 astride 4 KiB"))
        cases.append(Case(op, (np.where(L & 1, MEM_BYTES - 16, 0), 448, 0, _r32(rng)), mem=_mem(rng), note="first and last 16 bytes, last image slot"))
    for k, dst in enumerate((0, 4, 128, 200, 256)):
        cases.append(Case("GLDS16_S_TWO", (64 + k + 16 * L, dst, 4096 + 3 * k + 16 * rng.permutation(64)), mem=_mem(rng),
                          note="two images from dword %d" % dst))
    for k, dst in enumerate((0, 4, 64, 352, 704)):
        cases.append(Case("GLDS4_TOUCH", (k + 4 * rng.permutation(64) + (4090 if k == 4 else 32), dst), mem=_mem(rng), note="dump area at dword %d" % dst))
    return cases


FAMILIES = {"minima": minima, "sums": sums, "lane_moves": lane_moves, "words": words, "access": access, "atomics": atomics,
            "scalar_loads": scalar_loads, "lds_dma": lds_dma}


# ------------------------------------------------------------------------------------------------
def tin_inverse(e):
    """what to store so that the tight surroundings' input step yields e"""
    return np.where((L & 1)[:, None].astype(bool), e ^ U32(TIN_XOR), e - U32(TIN_ADD)).astype(U32)


def pack(cases, mode):
    """-> hdr (n, 4), inputs (n, 64, IN_W), mems (slots, MEM_BYTES); slot 0 belongs to the cases without memory"""
    hdr = np.zeros((len(cases), 4), dtype=U32)
    inputs = np.zeros((len(cases), 64, IN_W), dtype=U32)
    mems = [np.zeros(MEM_BYTES, dtype=np.uint8)]
    for k, c in enumerate(cases):
        inputs[k] = c.inp
        if mode == TIGHT:
            t = list(OPS[c.op][0])
            inputs[k][:, t] = tin_inverse(c.inp[:, t])
            inputs[k][:, IN_W - 1] = TIN_XOR                # tin's key, read from memory inside its branch
        if c.mem is not None:
            mems.append(c.mem)
        hdr[k] = (OP[c.op], mode, len(mems) - 1 if c.mem is not None else 0, 0)
    return hdr, inputs, np.stack(mems)


def check(cases, mode, nwaves, out, after):
    """out (n, nwaves, 64, OUT_W), after (slots, nwaves, MEM_BYTES): what a run of pack(cases, mode) gave.  Asserts that every wave
    of every case has the contract's results, bit for bit, and left its memory as the contract says."""
    hdr = pack(cases, mode)[0]
    if mode == TIGHT:                                       # every word of a case went through the xor of its operation
        key = np.array([TOUT_XOR ^ ((OP[c.op] * TOUT_MUL) & 0xFFFFFFFF) for c in cases], dtype=U32)
        out = out ^ key[:, None, None, None]
    assert not after[0].any(), "a case without memory of its own wrote into the memory it was handed"
    by_op = {}
    for k, c in enumerate(cases):
        by_op.setdefault(c.op, []).append(k)
    for op, ks in by_op.items():
        e = np.stack([cases[k].inp for k in ks])
        mem = np.stack([cases[k].mem for k in ks]) if cases[ks[0]].mem is not None else None
        exp = OPS[op][1](e, mem, nwaves)
        want = exp["out"] if exp["out"].ndim == 4 else np.repeat(exp["out"][:, None], nwaves, axis=1)
        got = out[ks].copy()
        if "olds" in exp:                                   # the old values: per word the same set, in any order of the lanes
            word, target = exp["olds"]
            key = np.repeat(target.astype(np.int64)[:, None], nwaves, axis=1) << 32
            g, w = np.sort(key | got[..., word], axis=-1), np.sort(key | want[..., word], axis=-1)
            bad = np.argwhere(g != w)
            assert len(bad) == 0, "%s, case %d (%s), wave %d: the old values are not the prefix sums in some order" % (
                op, bad[0][0], cases[ks[bad[0][0]]].note, bad[0][1])
            got[..., word] = want[..., word]
        bad = np.argwhere(got != want)
        if len(bad):
            i, w, lane, word = bad[0]
            raise AssertionError("%s %s, case %d (%s), wave %d of %d, lane %d, word %d: %#x, the contract says %#x (%d words differ in %d cases)" % (
                op, ("plain", "tight")[mode], i, cases[ks[i]].note, w, nwaves, lane, word, got[i, w, lane, word], want[i, w, lane, word],
                len(bad), len(set(bad[:, 0]))))
        if mem is not None:
            slots = hdr[ks, 2]
            want_mem = exp.get("mem", mem)
            bad = np.argwhere(after[slots] != want_mem[:, None, :])
            assert len(bad) == 0, "%s %s, case %d (%s), wave %d: byte %d of its memory is %#x, the contract says %#x" % (
                op, ("plain", "tight")[mode], bad[0][0], cases[ks[bad[0][0]]].note, bad[0][1], bad[0][2],
                after[slots][tuple(bad[0])], want_mem[bad[0][0], bad[0][2]])
