// prims_ops.h -- one routine per primitive of the interface of circkit_amd/csrc/wave_prims.h (TEST INFRASTRUCTURE ONLY, never
// linked into the product).  Written against the ck:: interface alone: the same text is compiled against the gfx950 device half
// (tests/prims/prims_probe.hip) and against the CPU fiber implementation (tests/emu/prims_emu_main.cpp), and both results are
// compared with the restatement of tests/prims_ref.py.  Whoever includes this has included wave_prims.h before.
//
// A case is one wave's work: every lane reads its input words (IN_W - 1 of them; the last is tin's), calls the primitive and
// writes every result the primitive defines for that lane into its OUT_W output words (words the routine does not write are 0).  All control flow around the
// primitives is wave-uniform: the operation and the mode are wave-uniform values, and every wave of a workgroup runs the same case.
// Two surroundings (MODE): plain -- the inputs come straight from a load and the results go straight into a store; tight -- a VALU
// operation computes every data input inside a lane-divergent `if` that reconverges in front of the primitive (tin), and a VALU
// operation consumes every result behind it, inside the operation's own case (fin).  tests/prims_sets.py stores the inverse of tin, so both modes run the same values.
// Memory a case may touch: MEM_BYTES of global memory of its own (`g`, wave-uniform), LDS_DW dwords of LDS of its own wave (`lds`),
// XCHG_DW dwords shared by the workgroup (`xchg`).  Every offset taken from the inputs is clamped into its region first.
#pragma once
#include <stdint.h>

namespace ck_prims {

constexpr uint32_t IN_W = 8, OUT_W = 16, LDS_DW = 768, MEM_BYTES = 8192, XCHG_DW = 16;
constexpr uint32_t LDS_FILL = 0xC0DE0000u;                  // dword k of an untouched LDS slice holds LDS_FILL + k
constexpr uint32_t TIN_XOR = 0x5A5A5A5Au, TIN_ADD = 0x01010101u, TOUT_XOR = 0x3C3C3C3Cu, TOUT_MUL = 0x9E3779B1u;
constexpr uint32_t DMA_TAIL = 704;                          // GLDS16's plain store and load: dword DMA_TAIL + lane

// (tests/prims_sets.py reads the names and their order from here)
enum Op : uint32_t {
    OP_IDS = 0,
    OP_BARRIER,
    OP_WAVE_MIN,
    OP_ROW_MIN16,
    OP_WAVE_MIN2,
    OP_HALF_MIN2,
    OP_HALF_MIN2_BCAST,
    OP_PK_MIN_U16,
    OP_ROWSUM4,
    OP_QUADSUM,
    OP_WAVE_SUM,
    OP_ADD64_PARTS,
    OP_MULHI64,
    OP_SHFL,
    OP_READLANE,
    OP_UNIFORM,
    OP_UNIFORM64,
    OP_WAVE_SHL1,
    OP_ROW_SHR_1,
    OP_ROW_SHR_2,
    OP_ROW_SHR_3,
    OP_ROW_SHR_4,
    OP_ROW_SHR_5,
    OP_ROW_SHR_6,
    OP_ROW_SHR_7,
    OP_ROW_SHR_8,
    OP_ROW_SHR_9,
    OP_ROW_SHR_10,
    OP_ROW_SHR_11,
    OP_ROW_SHR_12,
    OP_ROW_SHR_13,
    OP_ROW_SHR_14,
    OP_ROW_SHR_15,
    OP_QUAD_XOR1,
    OP_QUAD_XOR2,
    OP_HALF_BCAST,
    OP_BALLOT,
    OP_LANE_PRED,
    OP_FUNNEL,
    OP_ALIGNBIT,
    OP_LSHR64,
    OP_BFI,
    OP_BFI_V,
    OP_PERM,
    OP_BITREV,
    OP_FFS32,
    OP_FFS64,
    OP_CLZ32,
    OP_POPC32,
    OP_POPC64,
    OP_FFS32_OR_NEG,
    OP_FFS64_OR_NEG,
    OP_LOW_MASK16,
    OP_SAD_U8,
    OP_UDOT4,
    OP_LOAD16,
    OP_LOAD4,
    OP_STORE16,
    OP_STORE8,
    OP_STORE4,
    OP_LDS_RW16,
    OP_ATOMIC_ADD,
    OP_LDS_ATOMICS,
    OP_SLOAD_U64X2,
    OP_SLOAD_2U64,
    OP_SLOAD_GROUP_4,
    OP_SLOAD_GROUP_8,
    OP_SLOAD_GROUP_16,
    OP_GLDS16,
    OP_GLDS16_S,
    OP_GLDS16_S_TWO,
    OP_GLDS4_TOUCH,
    OP_COUNT
};

// (the odd lanes' key comes from memory -- the lane's last input word, TIN_XOR in the tight cases -- so that the `if` stays a branch
// under the execution mask instead of becoming a select)
template <int MODE>
CK_DEV uint32_t tin(const uint32_t* key, uint32_t v)
{
    if (MODE) {
        if (ck::lane_id() & 1) v ^= *key;
        else v += TIN_ADD;
    }
    return v;
}
// what the tight surroundings xor a result of operation `op` with: another word for every operation, so that the xor of one
// case is not the xor of the next and stays in the case's own block, directly behind its primitive
CK_DEV uint32_t tout_key(uint32_t op) { return TOUT_XOR ^ (op * TOUT_MUL); }
// the first N result words consumed, at the end of the operation's own case; returns N
// (in the gfx950 listing the xor is in the primitive's basic block, behind at most one scalar move of the structurized switch)
template <int MODE, uint32_t OP, uint32_t N>
CK_DEV uint32_t fin(uint32_t* o)
{
    if (MODE)
        for (uint32_t k = 0; k < N; ++k) o[k] ^= tout_key(OP);
    return N;
}

CK_DEV uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
CK_DEV void put64(uint32_t* o, uint64_t v) { o[0] = (uint32_t)v; o[1] = (uint32_t)(v >> 32); }
// a byte offset into the case's global memory at which `bytes` more still lie inside it
CK_DEV uint32_t in_mem(uint32_t off, uint32_t bytes) { return off <= MEM_BYTES - bytes ? off : MEM_BYTES - bytes; }
// the same, a multiple of `align` (a power of two)
CK_DEV uint32_t in_mem_al(uint32_t off, uint32_t bytes, uint32_t align) { return in_mem(off, bytes) & ~(align - 1u); }
// a dword index into the wave's LDS slice, a multiple of `align` dwords, with `dwords` more inside the first `end` dwords
CK_DEV uint32_t in_lds(uint32_t k, uint32_t dwords, uint32_t align, uint32_t end = LDS_DW)
{
    return (k <= end - dwords ? k : end - dwords) & ~(align - 1u);
}

// the wave's slice filled with its pattern, finished in LDS before anything else is issued (block_barrier: every wave of the
// workgroup runs the same case)
CK_DEV void lds_fill(uint32_t* lds)
{
    const uint32_t t = ck::lane_id();
    for (uint32_t j = 0; j < LDS_DW / 64; ++j) lds[(LDS_DW / 64) * t + j] = LDS_FILL + (LDS_DW / 64) * t + j;
    ck::block_barrier();
}
// the whole slice into o[0..11]: lane t takes dwords 12 t .. 12 t + 11
CK_DEV void lds_dump(const uint32_t* lds, uint32_t* o)
{
    const uint32_t t = ck::lane_id();
    ck::wave_sync();
    for (uint32_t j = 0; j < 3; ++j) {
        const ck::u32x4 v = ck::lds_load16(lds + 12 * t + 4 * j);
        o[4 * j] = v.x; o[4 * j + 1] = v.y; o[4 * j + 2] = v.z; o[4 * j + 3] = v.w;
    }
}

#define CK_PRIMS_ROW_SHR(N) case OP_ROW_SHR_##N: o[0] = ck::dpp_row_shr<N>(tin<MODE>(key, i[0])); return fin<MODE, OP_ROW_SHR_##N, 1>(o);

template <int GROUP, int MODE>
CK_DEV void op_sload_group(const uint32_t* i, uint32_t* o, const uint8_t* g)
{
    // p[0] and p[GROUP], q[0..2]: 8-byte aligned, inside the case's memory
    const uint64_t* p = (const uint64_t*)(g + in_mem_al(ck::uniform(i[0]), 8 * GROUP + 8, 8));
    const uint64_t* q = (const uint64_t*)(g + in_mem_al(ck::uniform(i[1]), 24, 8));
    uint64_t s, e, o0, o1, o2;
    ck::sload_group<GROUP>(p, q, s, e, o0, o1, o2);
    put64(o, s); put64(o + 2, e); put64(o + 4, o0); put64(o + 6, o1); put64(o + 8, o2);
}

// one lane's part of one case: key = tin's word, i = its inputs, o = its OUT_W results (zeroed by the caller)
template <int MODE>
CK_DEV uint32_t run_op(uint32_t op, const uint32_t* key, const uint32_t* i, uint32_t* o, uint8_t* g, uint32_t* lds, uint32_t* xchg, uint32_t nwaves)
{
    const uint32_t t = ck::lane_id();
    switch (op) {
    case OP_IDS: o[0] = ck::lane_id(); o[1] = ck::wave_in_block(); return fin<MODE, OP_IDS, 2>(o);
    case OP_BARRIER: {
        // every wave leaves a word, every wave reads them all behind the barrier
        if (t == 0) xchg[ck::wave_in_block()] = tin<MODE>(key, i[0]) + ck::wave_in_block();
        ck::block_barrier();
        uint32_t s = 0;
        for (uint32_t k = 0; k < XCHG_DW; ++k) s += k < nwaves ? xchg[k] : 0u;
        o[0] = s;
        return fin<MODE, OP_BARRIER, 1>(o);
    }
    // ---- minima
    case OP_WAVE_MIN: o[0] = ck::wave_min_u32(tin<MODE>(key, i[0])); return fin<MODE, OP_WAVE_MIN, 1>(o);
    case OP_ROW_MIN16: o[0] = ck::row_min16_u32(tin<MODE>(key, i[0])); return fin<MODE, OP_ROW_MIN16, 1>(o);
    case OP_WAVE_MIN2: ck::wave_min2_u32(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), o[0], o[1]); return fin<MODE, OP_WAVE_MIN2, 2>(o);
    case OP_HALF_MIN2: ck::half_min2_u32(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), o[0], o[1], o[2], o[3]); return fin<MODE, OP_HALF_MIN2, 4>(o);
    case OP_HALF_MIN2_BCAST: ck::half_min2_bcast_u32(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), o[0], o[1]); return fin<MODE, OP_HALF_MIN2_BCAST, 2>(o);
    case OP_PK_MIN_U16: o[0] = ck::pk_min_u16(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])); return fin<MODE, OP_PK_MIN_U16, 1>(o);
    // ---- 64-bit sums
    case OP_ROWSUM4: {
        uint64_t a = u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])), b = u64_of(tin<MODE>(key, i[2]), tin<MODE>(key, i[3]));
        ck::dpp_rowsum4_u64x2(a, b);
        put64(o, a); put64(o + 2, b);
        return fin<MODE, OP_ROWSUM4, 4>(o);
    }
    case OP_QUADSUM: put64(o, ck::dpp_quadsum_u64(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])))); return fin<MODE, OP_QUADSUM, 2>(o);
    case OP_WAVE_SUM: put64(o, ck::wave_sum_u64(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])))); return fin<MODE, OP_WAVE_SUM, 2>(o);
    case OP_ADD64_PARTS: put64(o, ck::add64_parts(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])), tin<MODE>(key, i[2]), tin<MODE>(key, i[3]))); return fin<MODE, OP_ADD64_PARTS, 2>(o);
    case OP_MULHI64: put64(o, ck::mulhi64(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])), u64_of(tin<MODE>(key, i[2]), tin<MODE>(key, i[3])))); return fin<MODE, OP_MULHI64, 2>(o);
    // ---- lane moves
    case OP_SHFL: o[0] = ck::shfl(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])); return fin<MODE, OP_SHFL, 1>(o);
    case OP_READLANE: o[0] = ck::readlane(tin<MODE>(key, i[0]), ck::uniform(i[1])); return fin<MODE, OP_READLANE, 1>(o);
    case OP_UNIFORM: o[0] = ck::uniform(tin<MODE>(key, i[0])); return fin<MODE, OP_UNIFORM, 1>(o);
    case OP_UNIFORM64: put64(o, ck::uniform64(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])))); return fin<MODE, OP_UNIFORM64, 2>(o);
    case OP_WAVE_SHL1: o[0] = ck::wave_shl1(tin<MODE>(key, i[0])); return fin<MODE, OP_WAVE_SHL1, 1>(o);
    CK_PRIMS_ROW_SHR(1) CK_PRIMS_ROW_SHR(2) CK_PRIMS_ROW_SHR(3) CK_PRIMS_ROW_SHR(4) CK_PRIMS_ROW_SHR(5)
    CK_PRIMS_ROW_SHR(6) CK_PRIMS_ROW_SHR(7) CK_PRIMS_ROW_SHR(8) CK_PRIMS_ROW_SHR(9) CK_PRIMS_ROW_SHR(10)
    CK_PRIMS_ROW_SHR(11) CK_PRIMS_ROW_SHR(12) CK_PRIMS_ROW_SHR(13) CK_PRIMS_ROW_SHR(14) CK_PRIMS_ROW_SHR(15)
    case OP_QUAD_XOR1: o[0] = ck::dpp_quad_xor1(tin<MODE>(key, i[0])); return fin<MODE, OP_QUAD_XOR1, 1>(o);
    case OP_QUAD_XOR2: o[0] = ck::dpp_quad_xor2(tin<MODE>(key, i[0])); return fin<MODE, OP_QUAD_XOR2, 1>(o);
    case OP_HALF_BCAST: ck::half_bcast(tin<MODE>(key, i[0]), o[0], o[1]); return fin<MODE, OP_HALF_BCAST, 2>(o);
    case OP_BALLOT: put64(o, ck::ballot((tin<MODE>(key, i[0]) & 1u) != 0)); return fin<MODE, OP_BALLOT, 2>(o);
    case OP_LANE_PRED: o[0] = ck::lane_pred(ck::uniform64(u64_of(i[0], i[1]))) ? 1u : 0u; return fin<MODE, OP_LANE_PRED, 1>(o);
    // ---- words
    case OP_FUNNEL: o[0] = ck::funnel(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2]) & 31u); return fin<MODE, OP_FUNNEL, 1>(o);
    case OP_ALIGNBIT: o[0] = ck::alignbit(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_ALIGNBIT, 1>(o);
    case OP_LSHR64: o[0] = ck::lshr64(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2]) & 63u); return fin<MODE, OP_LSHR64, 1>(o);
    case OP_BFI: o[0] = ck::bfi(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_BFI, 1>(o);
    case OP_BFI_V: o[0] = ck::bfi_v(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_BFI_V, 1>(o);
    case OP_PERM: o[0] = ck::perm(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_PERM, 1>(o);
    case OP_BITREV: o[0] = ck::bitrev(tin<MODE>(key, i[0])); return fin<MODE, OP_BITREV, 1>(o);
    // (ffs32, ffs64 and clz32 are defined for words other than 0 only)
    case OP_FFS32: { const uint32_t v = tin<MODE>(key, i[0]); o[0] = (uint32_t)ck::ffs32(v ? v : 1u); return fin<MODE, OP_FFS32, 1>(o); }
    case OP_FFS64: { const uint64_t v = u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1])); o[0] = (uint32_t)ck::ffs64(v ? v : 1u); return fin<MODE, OP_FFS64, 1>(o); }
    case OP_CLZ32: { const uint32_t v = tin<MODE>(key, i[0]); o[0] = (uint32_t)ck::clz32(v ? v : 1u); return fin<MODE, OP_CLZ32, 1>(o); }
    case OP_POPC32: o[0] = (uint32_t)ck::popc32(tin<MODE>(key, i[0])); return fin<MODE, OP_POPC32, 1>(o);
    case OP_POPC64: o[0] = (uint32_t)ck::popc64(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]))); return fin<MODE, OP_POPC64, 1>(o);
    case OP_FFS32_OR_NEG: o[0] = (uint32_t)ck::ffs32_or_neg(ck::uniform(i[0])); return fin<MODE, OP_FFS32_OR_NEG, 1>(o);             // a wave-uniform word
    case OP_FFS64_OR_NEG: o[0] = (uint32_t)ck::ffs64_or_neg(u64_of(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]))); return fin<MODE, OP_FFS64_OR_NEG, 1>(o);
    case OP_LOW_MASK16: o[0] = ck::low_mask16(ck::uniform(i[0])); return fin<MODE, OP_LOW_MASK16, 1>(o);                           // left is wave-uniform
    case OP_SAD_U8: o[0] = ck::sad_u8(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_SAD_U8, 1>(o);
    case OP_UDOT4: o[0] = ck::udot4(tin<MODE>(key, i[0]), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_UDOT4, 1>(o);
    // ---- global and LDS access: i[0] = the lane's byte offset into g
    case OP_LOAD16: { const ck::u32x4 v = ck::load16(g + in_mem(i[0], 16)); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; return fin<MODE, OP_LOAD16, 4>(o); }
    case OP_LOAD4: o[0] = ck::load4(g + in_mem(i[0], 4)); return fin<MODE, OP_LOAD4, 1>(o);
    case OP_STORE16: ck::store16(g + in_mem(i[0], 16), ck::u32x4{ tin<MODE>(key, i[1]), tin<MODE>(key, i[2]), tin<MODE>(key, i[3]), tin<MODE>(key, i[4]) }); return fin<MODE, OP_STORE16, 0>(o);
    case OP_STORE8: ck::store8(g + in_mem(i[0], 8), tin<MODE>(key, i[1]), tin<MODE>(key, i[2])); return fin<MODE, OP_STORE8, 0>(o);
    case OP_STORE4: ck::store4(g + in_mem(i[0], 4), tin<MODE>(key, i[1])); return fin<MODE, OP_STORE4, 0>(o);
    case OP_LDS_RW16: {
        // i[0]: dword index of the lane's 16 bytes (a multiple of 4), i[1..4]: what it stores, i[5]: where it loads from afterwards
        lds_fill(lds);
        ck::lds_store16(lds + in_lds(i[0], 4, 4), ck::u32x4{ tin<MODE>(key, i[1]), tin<MODE>(key, i[2]), tin<MODE>(key, i[3]), tin<MODE>(key, i[4]) });
        ck::wave_sync();
        const ck::u32x4 v = ck::lds_load16(lds + in_lds(i[5], 4, 4));
        lds_dump(lds, o);
        o[12] = v.x; o[13] = v.y; o[14] = v.z; o[15] = v.w;
        return fin<MODE, OP_LDS_RW16, 16>(o);
    }
    // ---- atomics
    case OP_ATOMIC_ADD: o[0] = ck::atomic_add_u32((uint32_t*)(g + in_mem_al(i[0], 4, 4)), tin<MODE>(key, i[1])); return fin<MODE, OP_ATOMIC_ADD, 1>(o);
    case OP_LDS_ATOMICS: {
        // four disjoint quarters of the slice, one per primitive: i[0], i[1], i[3], i[5] = dword index inside the quarter
        lds_fill(lds);
        constexpr uint32_t Q = LDS_DW / 4;
        const uint32_t old = ck::lds_atomic_inc(lds + in_lds(i[0], 1, 1, Q));
        ck::lds_atomic_or(lds + Q + in_lds(i[1], 1, 1, Q), tin<MODE>(key, i[2]));
        ck::lds_atomic_min(lds + 2 * Q + in_lds(i[3], 1, 1, Q), tin<MODE>(key, i[4]));
        ck::lds_atomic_add(lds + 3 * Q + in_lds(i[5], 1, 1, Q), tin<MODE>(key, i[6]));
        lds_dump(lds, o);
        o[12] = old;
        return fin<MODE, OP_LDS_ATOMICS, 16>(o);
    }
    // ---- scalar loads: wave-uniform 8-byte-aligned byte offsets into g, which nobody writes
    case OP_SLOAD_U64X2: {
        uint64_t a, b;
        ck::sload_u64x2((const uint64_t*)(g + in_mem_al(ck::uniform(i[0]), 16, 8)), a, b);
        put64(o, a); put64(o + 2, b);
        return fin<MODE, OP_SLOAD_U64X2, 4>(o);
    }
    case OP_SLOAD_2U64: {
        uint64_t a, b;
        ck::sload_2u64((const uint64_t*)(g + in_mem_al(ck::uniform(i[0]), 8, 8)), (const uint64_t*)(g + in_mem_al(ck::uniform(i[1]), 8, 8)), a, b);
        put64(o, a); put64(o + 2, b);
        return fin<MODE, OP_SLOAD_2U64, 4>(o);
    }
    case OP_SLOAD_GROUP_4: op_sload_group<4, MODE>(i, o, g); return fin<MODE, OP_SLOAD_GROUP_4, 10>(o);
    case OP_SLOAD_GROUP_8: op_sload_group<8, MODE>(i, o, g); return fin<MODE, OP_SLOAD_GROUP_8, 10>(o);
    case OP_SLOAD_GROUP_16: op_sload_group<16, MODE>(i, o, g); return fin<MODE, OP_SLOAD_GROUP_16, 10>(o);
    // ---- LDS-DMA: i[0] = the lane's source byte offset into g, i[1] = wave-uniform dword index of the image in the slice
    case OP_GLDS16: {
        // ... and a plain LDS store (i[3]) and a load of the neighbour's behind it, away from the image
        // (its value is made in front of the DMA: tin's load would otherwise bring a compiler's vmcnt(0) of its own)
        const uint32_t mine = tin<MODE>(key, i[3]);
        lds_fill(lds);
        ck::glds16_async(lds + in_lds(ck::uniform(i[1]), 256, 4, DMA_TAIL), g + in_mem(i[0], 16));
        lds[DMA_TAIL + t] = mine;
        ck::wave_sync();
        const uint32_t back = lds[DMA_TAIL + (t ^ 1u)];     // (the neighbour's: the compiler would forward the lane's own)
        ck::vmem_wait<0>();
        lds_dump(lds, o);
        o[12] = back;
        return fin<MODE, OP_GLDS16, 16>(o);
    }
    case OP_GLDS16_S: {
        lds_fill(lds);
        ck::glds16_async_s(lds + in_lds(ck::uniform(i[1]), 256, 4), g, in_mem(i[0], 16));
        ck::vmem_wait<0>();
        lds_dump(lds, o);
        return fin<MODE, OP_GLDS16_S, 16>(o);
    }
    case OP_GLDS16_S_TWO: {
        // two images back to back (the second from i[2]); with one DMA still allowed in flight the first is complete
        lds_fill(lds);
        uint32_t* first = lds + in_lds(ck::uniform(i[1]), 512, 4);
        ck::glds16_async_s(first, g, in_mem(i[0], 16));
        ck::glds16_async_s(first + 256, g, in_mem(i[2], 16));
        ck::vmem_wait<1>();
        ck::wave_sync();
        const ck::u32x4 v = ck::lds_load16(first + 4 * t);
        ck::vmem_wait<0>();
        lds_dump(lds, o);
        o[12] = v.x; o[13] = v.y; o[14] = v.z; o[15] = v.w;
        return fin<MODE, OP_GLDS16_S_TWO, 16>(o);
    }
    case OP_GLDS4_TOUCH: {
        // the dump area's 256 bytes at i[1]: lane t's four bytes land in dword t of it
        lds_fill(lds);
        ck::glds4_touch(lds + in_lds(ck::uniform(i[1]), 64, 4), g, in_mem(i[0], 4));
        ck::vmem_wait<0>();
        lds_dump(lds, o);
        return fin<MODE, OP_GLDS4_TOUCH, 16>(o);
    }
    default: o[0] = 0xBAD0BAD0u; return 0;
    }
}

// one lane's part of one case in its surroundings: load, primitive, store
template <int MODE>
CK_DEV void run_case(uint32_t op, const uint32_t* in, uint32_t* out, uint8_t* g, uint32_t* lds, uint32_t* xchg, uint32_t nwaves)
{
    uint32_t i[IN_W], o[OUT_W];
    for (uint32_t k = 0; k + 1 < IN_W; ++k) i[k] = in[k];
    i[IN_W - 1] = 0;                                        // the last word is tin's
    for (uint32_t k = 0; k < OUT_W; ++k) o[k] = 0;
    const uint32_t done = run_op<MODE>(op, in + (IN_W - 1), i, o, g, lds, xchg, nwaves);
    // (the words the case has not consumed itself -- zeros -- get the same xor, so that a tight result is one xor away from a plain one)
    for (uint32_t k = 0; k < OUT_W; ++k) out[k] = MODE && k >= done ? o[k] ^ tout_key(op) : o[k];
}

}  // namespace ck_prims
