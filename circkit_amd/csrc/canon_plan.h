// canon_plan.h -- the front of a batch (streaming kernel, rescue pass, mixed-length kernels) in one place: the words the ctx shares
// between host and kernels, which build owns a batch of a given mode, what a streaming build derives from its template
// parameters, the table of the front builds and the plan of a batch's front launches.  No kernel and no HIP
// runtime call, like canon_config.h: the kernels' early returns (canon_kernels.h) and the host's launch loop (circkit_canon.hip)
// call the same predicates, and tests/emu/emu.cpp exports them and the plan to tests/test_front_plan_cpu.py.
#pragma once
#include <stdint.h>

#include "canon_fast.h"
#include "canon_mixed.h"
#include "canon_config.h"

namespace {

// The words of the ctx's d_counters (32 x u32 of device memory, zero between batches unless noted).
enum CounterWord : uint32_t {
    CTR_PASSED_ON = 0,      // records the last LDS tier passed on: the global-scratch kernel's work
    CTR_TIERS_BUSY = 1,     // the rescue pass / the mixed kernel handed the tiers more than a record per segment
    CTR_GLOBAL_TICKET = 2,  // arrival ticket of the global-scratch kernel (leaves it zero)
    CTR_UNPROCESSED = 3,    // records nothing could take = CanonArgs::status[0]; adds up over the parts of a host batch
    CTR_ZEROED_PER_BATCH = 4,   // (a count: the words above, which a batch's first launch zeroes)
    CTR_MODE = 5,           // the batch's mode, when the device decides (stream_count_kernel)
    CTR_COUNT = 8,          // stream_count_kernel's control block, CountWord below (it leaves the block zero)
    CTR_POISON = 12,        // CK_DEBUG_POISON builds only (status[9] of canon_stream.h, never zeroed): the count block's unused word
    CTR_MIXED_TICKET = 16,  // [16] next segment, [17] workgroups through: the mixed N builds' ticket (self-zeroing)
    CTR_WORDS = 32,
};
enum CountWord : uint32_t { CNT_TWO_WORD = 0, CNT_LONGER = 1, CNT_TICKET = 2, CNT_NOT_ACGT = 3, CNT_UNUSED = 4, CNT_SHORT = 5 };
static_assert(CTR_COUNT + CNT_UNUSED == CTR_POISON && CTR_POISON == CTR_UNPROCESSED + 9, "the poison word sits in the count block's gap");
// The words of the ctx's pinned h_mode block (256 bytes, mapped: the device writes, the host reads without waiting).
enum HostWord : uint32_t {
    HM_MODE = 0,            // the mode of the batch that reported last (rescue pass / mixed kernel)
    HM_TIERS = 1,           // 1: that batch's tiers idled, 2: they worked (canon_global_kernel), 0: no batch yet
    HM_UNPROCESSED = 4,     // host_batch's copy of CTR_UNPROCESSED
};

// Ownership.  A batch's mode: bits 0..1 stream_mode, MODE_ALPHA, MODE_SHORT (batch_mode_of).  Exactly one streaming build takes
// a batch whose stream_mode is 1 or 2, none one of stream_mode 3; exactly one of the rescue and mixed builds takes any batch.
constexpr uint32_t N_MODES = 16;
CK_HD constexpr bool stream_owns(uint32_t rows, uint32_t rpw, bool hash, bool aux, bool alpha, uint32_t mode)
{
    if ((mode & 3) != rows) return false;                                       // the other build (or none) has this batch
    const bool has_alpha_twin = rows == 1 && !aux;
    if (has_alpha_twin && ((mode & MODE_ALPHA) != 0) != alpha) return false;
    if (has_alpha_twin && !alpha && !hash && ((mode & MODE_SHORT) != 0) != (rpw == 2)) return false;   // bytes only: the pair build has the batches of short records
    return true;
}
CK_HD constexpr bool rescue_owns(bool aux, bool alpha, uint32_t mode)
{
    if (!aux && ((mode & MODE_ALPHA) != 0) != alpha) return false;              // the other build has this batch
    if (!aux && (mode & 3) == 3) return false;                                  // ... or a canon_mixed kernel
    return true;
}
CK_HD constexpr bool mixed_owns(bool nm, uint32_t mode) { return (mode & 3) == 3 && ((mode & MODE_ALPHA) != 0) == nm; }

// What a streaming build derives from its template parameters (canon_stream_kernel; the emulator's stream_body).
template <class CFG, bool HASH, bool AUX, bool ALPHA>
struct StreamBuild {
    // GH: the fused XXH3 is finished per record group by one wave (canon_config.h CK_GROUP_HASH)
    static constexpr bool GH = CK_GROUP_HASH && HASH && !AUX && CFG::ROWS == 1 && (CFG::RPW == 1 || !ALPHA) && CFG::GROUP <= 16;
    static constexpr bool PAIR = GH && CFG::RPW == 2;                            // canon_pair.h: two records per wave
    static constexpr bool PAIR_B = !HASH && !AUX && !ALPHA && CFG::ROWS == 1 && CFG::RPW == 2;    // the bytes-only pair build: MODE_SHORT batches
    // min waves per SIMD the build is compiled for
    static constexpr int WPE = (HASH && !AUX && CFG::ROWS == 1 && (ALPHA || CFG::RPW == 2)) ? CK_PAIR_WPE : (CFG::WPB >= 8 || (ALPHA && !HASH && !AUX)) ? CK_FAST_WPE : 4;
    static constexpr uint32_t LDS_DW = CFG::LDS_DW + (GH ? ck::gh_lds_dw<(int)CFG::GROUP, PAIR>() : PAIR_B ? CFG::GROUP * ck::PAIR_SCRATCH_DW : 0);
    CK_HD static constexpr bool owns(uint32_t mode) { return stream_owns(CFG::ROWS, CFG::RPW, HASH, AUX, ALPHA, mode); }
};

// The front builds, in launch order: X(name, template arguments...).  The table below and circkit_canon.hip's kernel pointers
// expand the same lists.
//                    name           configuration HASH   AUX    ALPHA
#define CK_STREAM_BUILDS(X) \
    X(S_BYTES,        StreamC,       false, false, false) \
    X(S_BYTES_PAIR,   StreamCHP,     false, false, false) \
    X(S_BYTES_ALPHA,  StreamCA,      false, false, true)  \
    X(S_HASH_PAIR,    StreamCHP,     true,  false, false) \
    X(S_HASH_ALPHA,   StreamCH,      true,  false, true)  \
    X(S_AUX,          StreamCAux,    true,  true,  false) \
    X(S_TWO,          StreamC2,      false, false, false) \
    X(S_TWO_HASH,     StreamC2,      true,  false, false) \
    X(S_TWO_AUX,      StreamCAux2,   true,  true,  false)
#define CK_RESCUE_BUILDS(X) \
    X(R_AUX,          true,  true,  false) \
    X(R_HASH_LEAN,    true,  false, false) \
    X(R_HASH_ALPHA,   true,  false, true)  \
    X(R_BYTES_LEAN,   false, false, false) \
    X(R_BYTES_ALPHA,  false, false, true)
//                    name           kernel                 NM     HASH
#define CK_MIXED_BUILDS(X) \
    X(M_BYTES,        canon_mixed_kernel,    false, false) \
    X(M_BYTES_N,      canon_mixed_n_kernel,  true,  false) \
    X(M_HASH,         canon_mixed_h_kernel,  false, true)  \
    X(M_HASH_N,       canon_mixed_nh_kernel, true,  true)

#define CK_X(name, ...) name,
enum FrontBuildId : uint32_t { CK_STREAM_BUILDS(CK_X) CK_RESCUE_BUILDS(CK_X) CK_MIXED_BUILDS(CK_X) N_FRONT_BUILDS };
#undef CK_X
enum FrontStage : uint32_t { FRONT_STREAM, FRONT_RESCUE, FRONT_MIXED };
struct FrontBuild {
    const char* name;
    FrontStage stage;
    bool hash, aux, alpha;          // the template arguments (alpha: NM of a mixed build); aux, else hash: the batches it serves
    uint32_t rows, rpw;             // streaming builds: packed words per lane, records per wave
    uint32_t block;                 // workgroup size
    uint32_t slice_dw, lds;         // CanonArgs::slice_dw of the launch, dynamic LDS in bytes
};
// (the N builds keep one N bit per symbol and lean_resolve_n's candidates behind the strand: n / 16 + n / 32 + 24 dwords hold a
// 20 kb record of config 4 -- five workgroups = 20 waves per CU)
constexpr uint32_t mixed_slice_dw(bool nm) { return nm ? CK_MIXED_N_SLICE : TIER_DW[0]; }
constexpr uint32_t mixed_lds(bool nm, bool hash)
{
    return ((uint32_t)mixed_wpb(nm, hash) * mixed_slice_dw(nm) + 4 + ck::FAST_LUT_DW + ck::LEAN_LUTN_DW + (hash ? ck::LEAN_HASH_TABLE_DW : 0)) * 4;
}
constexpr FrontBuild FRONT_BUILDS[N_FRONT_BUILDS] = {
#define CK_X(id, CFG, HASH, AUX, ALPHA) { "canon_stream_kernel<" #CFG "," #HASH "," #AUX "," #ALPHA ">", FRONT_STREAM, HASH, AUX, ALPHA, CFG::ROWS, CFG::RPW, CFG::WPB * 64, 0, 0 },
    CK_STREAM_BUILDS(CK_X)
#undef CK_X
#define CK_X(id, HASH, AUX, ALPHA) { "canon_rescue_kernel<" #HASH "," #AUX "," #ALPHA ">", FRONT_RESCUE, HASH, AUX, ALPHA, 0, 0, 256, 0, 0 },
    CK_RESCUE_BUILDS(CK_X)
#undef CK_X
#define CK_X(id, KERNEL, NM, HASH) { #KERNEL, FRONT_MIXED, HASH, false, NM, 0, 0, 64 * mixed_wpb(NM, HASH), mixed_slice_dw(NM), mixed_lds(NM, HASH) },
    CK_MIXED_BUILDS(CK_X)
#undef CK_X
};
constexpr bool front_owns(const FrontBuild& b, uint32_t mode)
{
    return b.stage == FRONT_STREAM ? stream_owns(b.rows, b.rpw, b.hash, b.aux, b.alpha, mode)
         : b.stage == FRONT_RESCUE ? rescue_owns(b.aux, b.alpha, mode) : mixed_owns(b.alpha, mode);
}

// The plan of a batch's front launches.  A build is launched when it serves the batch's outputs and owns a mode the batch may
// still turn out to have: host_mode alone when the host knows (or guesses) it, every mode when the device decides.  A launched
// build gets its full-size grid exactly when it owns the mode the batch is expected to have -- host_mode, else the mode the
// last batch reported (`seen`, the pinned word read without waiting; stream_mode 1 while none has); the others get a small
// grid that walks the batch, return at once, and take the whole batch when the expectation was wrong.
struct FrontLaunch { uint32_t build; bool full; unsigned grid; };
struct FrontPlan { int n; FrontLaunch e[8]; };      // (at most four streaming builds, two behind them, two mixed)
constexpr uint32_t front_expected_mode(uint32_t host_mode, uint32_t seen)
{
    return host_mode ? host_mode & 15u : ((seen & 3u) ? seen & 15u : ((seen & 12u) | 1u));
}
constexpr unsigned front_grid(const FrontBuild& b, bool full, unsigned G, unsigned nseg)
{
    // the rescue pass's persistent grid, and the walking grid of a mixed build that is not expected to run
    const unsigned walking = nseg < (unsigned)N_CU * CK_RESCUE_BPC ? nseg : (unsigned)N_CU * CK_RESCUE_BPC;
    // mixed N builds: a resident grid (five workgroups per CU: 20 waves by LDS) fed by ticket; pure builds: one workgroup per segment
    const unsigned resident = (unsigned)N_CU * (20u / (unsigned)mixed_wpb(true, false));
    return b.stage == FRONT_STREAM ? (full || G < 2u * N_CU ? G : 2u * N_CU)
         : b.stage == FRONT_RESCUE || !full ? walking
         : b.alpha && resident < nseg ? resident : nseg;
}
inline FrontPlan canon_front_plan(bool aux, bool hash, uint32_t host_mode, uint32_t seen, unsigned G, unsigned nseg)
{
    const uint32_t expect = front_expected_mode(host_mode, seen);
    FrontPlan p{};
    for (uint32_t i = 0; i < N_FRONT_BUILDS; ++i) {
        const FrontBuild& b = FRONT_BUILDS[i];
        if (b.aux != aux || (!aux && b.hash != hash)) continue;
        bool launched = false;
        for (uint32_t m = 0; m < N_MODES; ++m) launched |= (!host_mode || m == (host_mode & 15u)) && front_owns(b, m);
        if (!launched) continue;
        const bool full = front_owns(b, expect);
        p.e[p.n++] = FrontLaunch{ i, full, front_grid(b, full, G, nseg) };
    }
    return p;
}

}  // namespace
