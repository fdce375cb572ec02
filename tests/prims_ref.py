"""The contract of every primitive of circkit_amd/csrc/wave_prims.h, restated in numpy on whole 64-lane arrays (tests only): one
short function per primitive, written from the comments of wave_prims.h and tests/emu/wave_prims_emu.h and from what the
instructions are documented to do, calling neither.  The lanes are the LAST axis (64); leading axes are independent waves.  A
result that is wave-uniform comes back in every lane.  32-bit values are uint32 arrays, 64-bit values uint64 arrays; sums wrap.

Memory: `mem` is (..., MEM) uint8, one image per wave; a store returns the new image.  LDS: (..., DW) uint32 per wave."""
import numpy as np

U32, U64 = np.uint32, np.uint64
L = np.arange(64)
M32 = U64(0xFFFFFFFF)


def _u32(v):
    return np.asarray(v).astype(U32)


def _u64(v):
    return np.asarray(v).astype(U64)


def _all(v, like):
    """a per-wave value in every lane"""
    return np.broadcast_to(np.asarray(v)[..., None], like.shape).copy()


def _take(v, src):
    return np.take_along_axis(v, np.broadcast_to(np.asarray(src, dtype=np.int64), v.shape), -1)


def _bits(v, n):
    return ((_u64(v)[..., None] >> np.arange(n, dtype=U64)) & U64(1)).astype(np.int64)


def _cat64(hi, lo):
    return (_u64(hi) << U64(32)) | _u64(lo)


# ---- who am I, and the points at which a wave or a workgroup meets (no value)
def lane_id(like):
    return np.broadcast_to(L.astype(U32), like.shape).copy()


def wave_in_block(w, like):
    """the wave's index in its workgroup, 0..15, wave-uniform"""
    return np.full(like.shape, w, dtype=U32)


def block_barrier():
    """every thread of the workgroup arrives before one leaves; what was written in front is visible behind"""


def wave_sync():
    """the wave's LDS traffic in front stays in front"""


def vmem_wait(n):
    """returns once at most n of the wave's vector-memory instructions -- LDS-DMA included, in issue order -- are outstanding"""


# ---- lane moves
def ballot(p):
    m = np.bitwise_or.reduce((np.asarray(p) != 0).astype(U64) << L.astype(U64), axis=-1)
    return _all(m, np.asarray(p))


def shfl(v, src):
    """the value of lane src mod 64"""
    return _take(_u32(v), _u32(src) & U32(63))


def readlane(v, lane):
    """lane: wave-uniform, 0..63"""
    return _take(_u32(v), _u32(lane)[..., :1] & U32(63))


def uniform(v):
    """the value of the first lane, in scalar registers"""
    return _all(_u32(v)[..., 0], _u32(v))


def uniform64(v):
    return _all(_u64(v)[..., 0], _u64(v))


def wave_shl1(v):
    """lane i <- lane i + 1, lane 63 <- 0"""
    v = _u32(v)
    return np.concatenate([v[..., 1:], np.zeros_like(v[..., :1])], -1)


def dpp_row_shr(v, n):
    """lane i - n of the same row of 16, 0 where that lane does not exist"""
    return np.where((L & 15) >= n, _u32(v)[..., np.maximum(L - n, 0)], U32(0))


def dpp_quad_xor1(v):
    return _u32(v)[..., L ^ 1]


def dpp_quad_xor2(v):
    return _u32(v)[..., L ^ 2]


def half_bcast(v):
    """(lo, hi): the lower / the upper half of the wave shown to both halves"""
    v = _u32(v)
    return v[..., L & 31], v[..., 32 + (L & 31)]


def lane_pred(m, like):
    """m: (...,) uint64, wave-uniform -> bit `lane` of it"""
    return ((_u64(m)[..., None] >> L.astype(U64)) & U64(1)).astype(bool)


# ---- minima (unsigned)
def wave_min_u32(v):
    return _all(_u32(v).min(-1), _u32(v))


def row_min16_u32(v):
    v = _u32(v)
    return np.repeat(v.reshape(v.shape[:-1] + (4, 16)).min(-1), 16, axis=-1)


def wave_min2_u32(x, y):
    return wave_min_u32(x), wave_min_u32(y)


def half_min2_u32(x, y):
    """(xa, xb, ya, yb): the minimum of lanes 0..31 and of lanes 32..63, of x and of y, all wave-uniform"""
    x, y = _u32(x), _u32(y)
    return _all(x[..., :32].min(-1), x), _all(x[..., 32:].min(-1), x), _all(y[..., :32].min(-1), y), _all(y[..., 32:].min(-1), y)


def half_min2_bcast_u32(x, y):
    """every lane gets the minimum of its own half"""
    xa, xb, ya, yb = half_min2_u32(x, y)
    return np.where(L < 32, xa, xb), np.where(L < 32, ya, yb)


def pk_min_u16(a, b):
    a, b = _u32(a), _u32(b)
    return (np.minimum(a >> U32(16), b >> U32(16)) << U32(16)) | np.minimum(a & U32(0xFFFF), b & U32(0xFFFF))


# ---- 64-bit sums (mod 2^64)
def dpp_rowsum4_u64x2(a, b):
    """lane i += lane i - 4, then += lane i - 8 of its row of 16; lanes that do not exist add 0"""
    def one(v):
        v = _u64(v)
        for step in (4, 8):
            v = v + np.where((L & 15) >= step, v[..., np.maximum(L - step, 0)], U64(0))
        return v
    return one(a), one(b)


def dpp_quadsum_u64(a):
    a = _u64(a)
    return a.reshape(a.shape[:-1] + (16, 4)).sum(-1, dtype=U64).repeat(4, axis=-1)


def wave_sum_u64(v):
    return _all(_u64(v).sum(-1, dtype=U64), _u64(v))


def add64_parts(a, lo, hi):
    return _u64(a) + _cat64(hi, lo)


def mulhi64(a, b):
    p = _u64(a).astype(object) * _u64(b).astype(object)
    return (p >> 64).astype(U64)


# ---- words
def lshr64(hi, lo, s):
    """low 32 bits of (hi:lo) >> s, s in 0..63"""
    return ((_cat64(hi, lo) >> _u64(s)) & M32).astype(U32)


def bfi(mask, a, b):
    return (_u32(mask) & _u32(a)) | (~_u32(mask) & _u32(b))


bfi_v = bfi


def perm(s0, s1, sel):
    """v_perm_b32: result byte i is byte sel_i of the eight bytes s0:s1 for sel_i in 0..7, 0x00 for 0x0c, 0xff from 0x0d on.
    Selectors 8..11 (sign replication) are outside the contract."""
    src = _cat64(s0, s1)
    r = np.zeros(src.shape, dtype=U32)
    for i in range(4):
        k = (_u32(sel) >> U32(8 * i)) & U32(0xFF)
        assert not ((k >= 8) & (k <= 11)).any(), "selectors 8..11 are outside the contract"
        byte = ((src >> (_u64(k & U32(7)) * U64(8))) & U64(0xFF)).astype(U32)
        r |= np.where(k <= 7, byte, np.where(k == 12, U32(0), U32(0xFF))) << U32(8 * i)
    return r


def funnel(hi, lo, sh):
    """the 32 bits that start sh bits (0..31) into hi:lo, counted from the top"""
    return (((_cat64(hi, lo) << _u64(sh)) >> U64(32)) & M32).astype(U32)


def alignbit(hi, lo, s):
    """low 32 bits of (hi:lo) >> (s mod 32)"""
    return ((_cat64(hi, lo) >> (_u64(s) & U64(31))) & M32).astype(U32)


def bitrev(v):
    return (_bits(v, 32)[..., ::-1] << np.arange(32)).sum(-1).astype(U32)


def ffs32(v):
    """index of the lowest set bit, v != 0"""
    return _bits(v, 32).argmax(-1).astype(U32)


def ffs64(v):
    return _bits(v, 64).argmax(-1).astype(U32)


def clz32(v):
    """zeros above the highest set bit, v != 0"""
    return _bits(v, 32)[..., ::-1].argmax(-1).astype(U32)


def popc32(v):
    return _bits(v, 32).sum(-1).astype(U32)


def popc64(v):
    return _bits(v, 64).sum(-1).astype(U32)


def ffs32_or_neg(v):
    """ffs32, and -1 for 0"""
    return np.where(_u32(v) == 0, U32(0xFFFFFFFF), ffs32(v))


def ffs64_or_neg(v):
    return np.where(_u64(v) == 0, U32(0xFFFFFFFF), ffs64(v))


def low_mask16(left):
    """the low min(left, 16) bits set"""
    return ((U32(1) << np.minimum(_u32(left), U32(16))) - U32(1)).astype(U32)


def _bytes(v):
    return [((_u32(v) >> U32(8 * k)) & U32(0xFF)).astype(np.int64) for k in range(4)]


def sad_u8(a, b, acc):
    return (_u32(acc).astype(np.int64) + sum(abs(x - y) for x, y in zip(_bytes(a), _bytes(b)))).astype(U64).astype(U32)


def udot4(a, b, c):
    """sum of the four byte products + c, mod 2^32"""
    return ((_u32(c).astype(np.int64) + sum(x * y for x, y in zip(_bytes(a), _bytes(b)))) & 0xFFFFFFFF).astype(U32)


# ---- global and LDS access: any byte offset for global memory, 16-byte-aligned for LDS
def _gather(mem, off, n):
    """n bytes per lane from byte offset off (..., 64) of mem (..., MEM)"""
    idx = np.asarray(off, dtype=np.int64)[..., None] + np.arange(n)
    return np.take_along_axis(mem[..., None, :], idx, -1)


def _scatter(mem, off, data):
    """a copy of mem with data (..., 64, n) uint8 written at the lanes' byte offsets (the lanes' ranges are disjoint)"""
    out = mem.copy()
    idx = np.asarray(off, dtype=np.int64)[..., None] + np.arange(data.shape[-1])
    flat = idx.reshape(idx.shape[:-2] + (-1,))
    np.put_along_axis(out, flat, data.reshape(flat.shape), -1)
    return out


def _words(b):
    """(..., 4 k) uint8 -> (..., k) little-endian uint32"""
    return np.ascontiguousarray(b).view(U32)


def _as_bytes(w):
    return np.ascontiguousarray(_u32(w)).view(np.uint8)


def load16(mem, off):
    """(..., 64, 4) uint32"""
    return _words(_gather(mem, off, 16))


def load4(mem, off):
    return _words(_gather(mem, off, 4))[..., 0]


def store16(mem, off, v):
    """v: (..., 64, 4)"""
    return _scatter(mem, off, _as_bytes(v))


def store8(mem, off, a, b):
    return _scatter(mem, off, _as_bytes(np.stack([_u32(a), _u32(b)], -1)))


def store4(mem, off, a):
    return _scatter(mem, off, _as_bytes(_u32(a)[..., None]))


def lds_load16(lds, k):
    """k: dword index (..., 64), a multiple of 4 -> (..., 64, 4)"""
    return np.take_along_axis(lds[..., None, :], np.asarray(k, dtype=np.int64)[..., None] + np.arange(4), -1)


def lds_store16(lds, k, v):
    out = lds.copy()
    idx = (np.asarray(k, dtype=np.int64)[..., None] + np.arange(4))
    np.put_along_axis(out, idx.reshape(idx.shape[:-2] + (-1,)), _u32(v).reshape(idx.shape[:-2] + (-1,)), -1)
    return out


# ---- atomics: the words afterwards, and for the ones that return it the SET of old values per word (the order of the lanes is free)
def _accumulate(words, k, v, fn):
    out = words.copy()
    k = np.broadcast_to(np.asarray(k, dtype=np.int64), np.asarray(v).shape)
    for lane in range(64):
        cur = np.take_along_axis(out, k[..., lane:lane + 1], -1)
        np.put_along_axis(out, k[..., lane:lane + 1], fn(cur, _u32(v)[..., lane:lane + 1]).astype(U32), -1)
    return out


def _olds(words, k, v):
    """what the lanes get back when they add in lane order: one of the allowed orders"""
    out, olds = words.copy(), np.zeros(np.asarray(v).shape, dtype=U32)
    k = np.broadcast_to(np.asarray(k, dtype=np.int64), olds.shape)
    for lane in range(64):
        cur = np.take_along_axis(out, k[..., lane:lane + 1], -1)
        olds[..., lane:lane + 1] = cur
        np.put_along_axis(out, k[..., lane:lane + 1], cur + _u32(v)[..., lane:lane + 1], -1)
    return olds


def atomic_add_u32(words, k, v):
    """words (..., W) uint32, k: the lanes' word index -> (words afterwards, old values in lane order)"""
    return _accumulate(words, k, v, lambda c, x: c + x), _olds(words, k, v)


def lds_atomic_inc(words, k):
    one = np.ones(np.asarray(k).shape, dtype=U32)
    return _accumulate(words, k, one, lambda c, x: c + x), _olds(words, k, one)


def lds_atomic_or(words, k, v):
    return _accumulate(words, k, v, lambda c, x: c | x)


def lds_atomic_min(words, k, v):
    return _accumulate(words, k, v, np.minimum)


def lds_atomic_add(words, k, v):
    return _accumulate(words, k, v, lambda c, x: c + x)


# ---- scalar loads: wave-uniform 8-byte-aligned byte offsets (...,) into memory nobody writes
def _u64_at(mem, off):
    idx = np.asarray(off, dtype=np.int64)[..., None] + np.arange(8)
    return np.ascontiguousarray(np.take_along_axis(mem, idx, -1)).view(U64)[..., 0]


def sload_u64x2(mem, p):
    """p[0], p[1]"""
    return _u64_at(mem, p), _u64_at(mem, np.asarray(p, dtype=np.int64) + 8)


def sload_2u64(mem, p0, p1):
    return _u64_at(mem, p0), _u64_at(mem, p1)


def sload_group(mem, p, q, span):
    """p[0], p[span], q[0], q[1], q[2]"""
    p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    return _u64_at(mem, p), _u64_at(mem, p + 8 * span), _u64_at(mem, q), _u64_at(mem, q + 8), _u64_at(mem, q + 16)


# ---- LDS-DMA: lane t's bytes land at dst + 16 t (4 t for the touch), complete once vmem_wait has let them through
def glds16_async(lds, dst, mem, off):
    """lds (..., DW), dst: wave-uniform dword index (...,), off: the lanes' source byte offsets"""
    k = np.asarray(dst, dtype=np.int64)[..., None] + 4 * L
    return lds_store16(lds, k, load16(mem, off))


def glds16_async_s(lds, dst, mem, voff):
    """the same with the source as a wave-uniform base + the lanes' offsets"""
    return glds16_async(lds, dst, mem, voff)


def glds4_touch(lds, dst, mem, voff):
    out = lds.copy()
    k = np.asarray(dst, dtype=np.int64)[..., None] + L
    np.put_along_axis(out, k, load4(mem, voff), -1)
    return out
