// canon_config.h -- the canonicalize unit's tuning in one place: the value knobs, the streaming kernel's configurations, the LDS
// stages' slice tables, the rules that name a batch's mode and the geometry of a batch's launches.  No kernel and no HIP runtime
// call: canon_kernels.h and circkit_canon.hip build on it, ck_ctx_impl.h sizes the ctx's lists by it, and the CPU emulator
// (tests/emu/emu.cpp) compiles it with the host compiler, so the tests run this arithmetic instead of restating it.
// Everything has internal linkage, like the kernels it configures (their symbol names do not depend on who includes this).
#pragma once
#include <stdint.h>

#include "canon_core.h"
#include "canon_stream.h"

#ifdef __HIPCC__
#define CK_HD __host__ __device__
#else
#define CK_HD
#endif

namespace {

#ifndef CK_FAST_WPE
#define CK_FAST_WPE 8    // min waves per SIMD the streaming kernel is compiled for (two 16-wave workgroups per CU: <= 64 VGPRs)
#endif
#ifndef CK_STREAM_WPB
#define CK_STREAM_WPB 16     // waves per workgroup of the staged streaming kernel
#endif
#ifndef CK_STREAM_NBUF
#define CK_STREAM_NBUF 2     // LDS images per workgroup (NBUF-1 groups in flight); 2 x 32 KiB, two 16-wave workgroups per CU
#endif
#ifndef CK_FAST_BPC
#define CK_FAST_BPC 128   // workgroups launched per CU (4-6 resident; the rest queue: finer dynamic balance)
#endif
#ifndef CK_TIER_WPE
#define CK_TIER_WPE 7      // min waves per SIMD the LDS-tier kernels are compiled for: 72 VGPRs, no spills (measured: 1 -> 76 VGPRs / 6 waves +2.7 %, 8 -> spills +1.2 %)
#endif
constexpr int TEAM_WAVES = 16;      // waves per workgroup of the last LDS stage and of the global-scratch stage (canon_team_kernel, canon_global_kernel)
// The streaming kernel with workgroup-staged input (canon_stream.h): a ring of images of record groups per
// workgroup, the decode table and the deferral counter.
#ifndef CK_STREAM_RPW
#define CK_STREAM_RPW 1      // records per wave per group
#endif
// Two builds of every streaming kernel: ROWS = 1 takes records of 48..1008 bases (one packed word per lane), ROWS = 2
// also 1009..2032 (two words per lane, 2 KiB of image per record); it is used when at least one record in four is
// such a record.  Carrying
// the two-word path makes the one-word path ~12 % longer, hence two builds.  Who decides: the host when it has the
// offsets (host-buffer API); otherwise the device, for every batch anew: stream_count_kernel counts the batch's
// lengths and every kernel derives the mode from the counters (batch_mode).  The call stays asynchronous: BOTH builds
// are launched, the one the previous batch used with a full grid, the other with a small one -- until the batches before
// have reported the same mode twice: then only that mode's build is launched (launch_canon, MODE_GUESS).
using StreamC = ck::StreamCfg<CK_STREAM_WPB, CK_STREAM_NBUF, CK_STREAM_RPW, 1>;
// (the two-word build in 8-wave workgroups, four per CU: 9 GB batches of 1.2 / 1.5 / 2 kb records 5.11 / 4.50 / 3.82 -> 4.98 / 4.32 / 3.76 ms)
#ifndef CK_STREAM_WPB_2
#define CK_STREAM_WPB_2 8
#endif
using StreamC2 = ck::StreamCfg<CK_STREAM_WPB_2, CK_STREAM_NBUF, CK_STREAM_RPW, 2>;
// The builds with the fused XXH3 (ROWS = 1) run 8-wave workgroups, four per CU, groups of 8 records (round 4): they are bound by
// instruction issue, and four independent barrier domains per CU leave fewer issue slots empty than two -- hash only -3 % on
// every box measured, bytes + hash -2 % .. 0.  The bytes-only builds are bound by the memory system and keep 16 waves (-1 % on one
// box, +3.5 % on another).
#ifndef CK_STREAM_WPB_HASH
#define CK_STREAM_WPB_HASH 4
#endif
using StreamCH = ck::StreamCfg<CK_STREAM_WPB_HASH, CK_STREAM_NBUF, CK_STREAM_RPW, 1>;
// ... and, for batches of pure ACGT, take TWO records per wave, one per half-wave (canon_pair.h): the scalar side of an iteration
// and the vector work that does not depend on the bytes are shared by two records.  CK_STREAM_WPB_PAIR waves, groups of twice as
// many records; CK_PAIR_WPE waves per SIMD (the register budget the build is compiled for).  CK_STREAM_WPB_PAIR 0: no such build.
// The bytes-only N build (MODE_ALPHA batches): 4 waves.  A record with an N among the symbols that decide (one in
// thirteen at 1 % N) takes the 4-bit routine behind the N-mask routine -- twice the work --, and the workgroup's barrier makes every
// wave wait for it: with 16 waves 72 % of the iterations hold such a record, with 8 waves 47 %, with 4 waves 27 % (10M x 1 kb, 1 % N, one
// box: 16 waves 4.90 ms, 8 waves 4.65, 4 waves 4.56, 2 waves 4.70).
#ifndef CK_STREAM_WPB_ALPHA
#define CK_STREAM_WPB_ALPHA 4
#endif
using StreamCA = ck::StreamCfg<CK_STREAM_WPB_ALPHA, CK_STREAM_NBUF, CK_STREAM_RPW, 1>;
#ifndef CK_STREAM_WPB_PAIR
#define CK_STREAM_WPB_PAIR 8
#endif
#ifndef CK_PAIR_WPE
#define CK_PAIR_WPE 6
#endif
#if CK_STREAM_WPB_PAIR
using StreamCHP = ck::StreamCfg<CK_STREAM_WPB_PAIR, CK_STREAM_NBUF, 2, 1>;
#else
using StreamCHP = StreamCH;
#endif
// The build with every output (index / strand / forward-only) needs ~100 SGPRs: at 16 waves per workgroup only one
// workgroup would fit a CU (measured: 5.1-5.7 ms instead of 3.4-4.0).  It keeps 4-wave workgroups (2 records per
// wave), where SGPRs only cost a seventh wave per SIMD.
using StreamCAux = ck::StreamCfg<4, 4, 2, 1>;
using StreamCAux2 = ck::StreamCfg<4, 2, 2, 2>;

// The ROWS = 2 build is used when at least 1 record in 4 is a 1009..2032-base one (it runs the shorter records 4-6 %
// slower, the longer ones 1.5x faster than LDS tier A; at 15 % -- BASELINE config 4 -- it measured 2 % slower overall).
// The decision is taken again for EVERY batch from the batch's own offsets (an earlier version remembered it per
// offsets pointer, which a host that reuses one offsets buffer defeats) -- from a SAMPLE of them: every mode computes
// the same results, the choice only has to be right about which is fastest, and reading all 80 MB of a 10M-record
// batch's offsets cost 16-21 us per batch.  Every 2^count_shift(n)-th record is looked at (<= 128k of them).
CK_HD inline uint32_t count_shift(uint64_t n) { return n <= (1u << 17) ? 0u : (uint32_t)(63 - __builtin_clzll(n)) - 16u; }
CK_HD inline uint64_t count_samples(uint64_t n) { return (n + (1ull << count_shift(n)) - 1) >> count_shift(n); }
// 1 / 2: which build of the streaming kernel; 3: neither -- with one record in eight longer than 2032 bases at most
// 12 % of the 16-record groups could be staged, and the rescue pass takes every record straight away
CK_HD inline uint32_t stream_mode(uint64_t two, uint64_t lng, uint64_t n)
{
    return lng && lng * 8 >= n ? 3u : (two && two * 4 >= n ? 2u : 1u);
}
// The same kernel samples the CONTENT: up to CONTENT_SAMPLES evenly spaced records, a wave each, first 1008 bytes -- does
// the record hold a byte outside ACGT?  With one sampled record in 16 (or more) doing so, the batch's mode carries
// MODE_ALPHA and the rescue pass runs its build with the 4-bit register path (canon_stream.h); otherwise the lean build,
// which leaves the odd N-bearing record to the LDS tiers (carrying the 4-bit path costs the lean one 25-45 %, measured).
constexpr uint32_t CONTENT_SAMPLES = 4096, MODE_ALPHA = 4;
// MODE_SHORT (mode 1, no MODE_ALPHA): most of the batch's records are short -- the bytes-only streaming kernel then runs its pair
// build (two records per wave, canon_pair.h); records of up to SHORT_MAX_N symbols count as short, half of the samples make the mode
constexpr uint32_t MODE_SHORT = 8, SHORT_MAX_N = 800;
CK_HD inline uint32_t alpha_mode(uint64_t bad, uint64_t sampled) { return bad && bad * 16 >= sampled ? MODE_ALPHA : 0u; }
// The batch's mode from the samples.  The two-word build of the streaming kernel has no alphabet twin -- its records with an N went
// to LDS stage A one by one (6M x 1.5 kb with 1 % N: 11.9 ms, 0.19 of peak) --, the mixed-length kernels have one: a batch of
// two-word records WITH N is theirs (mode 3).
// ... and so is one whose XXH3 is wanted (hashed: hashes and no index / strand): the two-word build finishes every record's hash by
// itself (fast_hash2: two blocks, a scramble between them), the mixed-length kernels with the XXH3 are 8-11 % faster on such batches
// (6M x 1.5 kb: 6.69 -> 6.12 ms; bytes only the two-word build wins, 4.45 against 4.74).
CK_HD inline uint32_t batch_mode_of(uint64_t two, uint64_t lng, uint64_t n, uint64_t bad, uint64_t sampled, uint64_t shortc, bool hashed)
{
    const uint32_t m = stream_mode(two, lng, n), al = alpha_mode(bad, sampled);
    return (m == 2 && (al || hashed) ? 3u : m) | al | (m == 1 && !al && shortc * 2 >= n ? MODE_SHORT : 0u);
}
// Waves per workgroup of the mixed-length kernels (a slice of LDS each; a workgroup takes one list segment -- ~30 records of config 4 --
// and leaves when its slowest wave does).  Measured on config 4, same box, 24 waves per CU in every case (tools/probe_variants.py):
// bytes only 1 / 2 / 4 / 8 waves 1.90 / 1.88 / 1.81 / 1.75 ms, with the XXH3 2.17 / 2.11 / 2.20 / 2.52.  The N builds' resident grid
// is sized for four.
#ifndef CK_MIXED_WPB_PURE
#define CK_MIXED_WPB_PURE 8
#endif
#ifndef CK_MIXED_WPB_HASH
#define CK_MIXED_WPB_HASH 2
#endif
#ifndef CK_MIXED_WPB_N
#define CK_MIXED_WPB_N 4
#endif
constexpr int mixed_wpb(bool nm, bool hash) { return nm ? CK_MIXED_WPB_N : (hash ? CK_MIXED_WPB_HASH : CK_MIXED_WPB_PURE); }
#ifndef CK_MIXED_NM_VGPR
#define CK_MIXED_NM_VGPR 48       // the N builds: five workgroups per CU by LDS (strand + N bits) = five waves per SIMD: 96 registers each
#endif
#ifndef CK_MIXED_H_VGPR
#define CK_MIXED_H_VGPR 40       // the builds with the fused XXH3: 80 registers, six waves per SIMD
#endif
#ifndef CK_MIXED_N_SLICE
#define CK_MIXED_N_SLICE 1904     // dwords per wave of the N builds: strand + N bits + candidates of a 20 kb record (1253 + 628 + 18); five workgroups per CU by LDS
#endif
// GH: the fused XXH3 is finished per 16-record group by one wave (canon_fast.h group_hash_*): 18.2 KiB more LDS, which
// the ROWS = 2 build cannot afford next to its 64 KiB of images (two workgroups per CU are what matters most).
#ifndef CK_GROUP_HASH
#define CK_GROUP_HASH 1
#endif
// ------------------------------------------------------------------------------------------------
// LDS stages of a batch behind the rescue pass (+ 276 dwords per workgroup: deferral counter, decode table, N patch table).
// A 2-bit record needs its ONE stored strand, n / 16 + 2 dwords (+ n / 32 for the candidate bitmask only if the minimal key
// ties); with a few N the strand + n / 32 of N bitmask; 4-bit and byte mode two strands + the bitmask.  In every stage a
// record goes to ONE wave if it fits that wave's slice, to the workgroup's waves as a TEAM if it is 2-bit material and fits
// their slices together, else to wave 0 ALONE with the workgroup's whole LDS (canon_core.h team_pass, canon_team_kernel).
//   A: 4 waves x 5 KiB (7 workgroups per CU)      one wave: 2-bit up to ~20.4 kb (all of BASELINE config 4), few N ~13.6 kb,
//                                                 4-bit ~8.2 kb (one stored strand since round 3); team: 2-bit ~81 kb, few N ~54 kb, 4-bit ~41 kb; alone: 4-bit ~33 kb
//   C: 4 waves x 9.7 KiB (4 workgroups per CU)    team: 2-bit up to ~160 kb, few N ~106 kb, 4-bit ~80 kb; alone: 4-bit ~64 kb, bytes ~17 kb
//   team stage: 16 waves x 157 KiB (the CU)       team: 2-bit up to ~640 kb, few N ~420 kb, 4-bit ~320 kb; alone: 4-bit ~250 kb, bytes ~70 kb
//   beyond: canon_global_kernel, the same over slices of a global-memory scratch (one more launch of every batch)
// (One-wave slices of 7.4 / 13 / 39 / 157 KiB -- stages of their own in earlier versions -- remain for single-record calls.)
#ifndef CK_RESCUE_BPC
#define CK_RESCUE_BPC 8      // workgroups per CU of the rescue pass's persistent grid
#endif
#ifndef CK_TIER_BPC
#define CK_TIER_BPC 128    // workgroups launched per CU by the LDS tiers at most (they walk the list segments); 128 = one per segment
#endif
#ifndef CK_TIER_BPC_IDLE
#define CK_TIER_BPC_IDLE 8 // ...when the previous batch left them (next to) nothing to do
#endif
// A 2-bit record is admitted by its one stored strand alone, (n + 15) / 16 + 2 dwords (the candidate bitmask is only needed
// on a tie of the minimal key; a record that ties without room for it moves on).  Tier A: 5 KiB per wave = records up to
// 20.4 kb -- all of BASELINE config 4 in the four-wave tier, 7 workgroups = 28 waves per CU by LDS and by VGPRs alike (6 by SGPRs for the mixed-length kernels, see there)
// (measured on config 4, one box: A = 4 KiB + B1 = 7.4 KiB with the bitmask counted in 2.41 ms, without it 2.30,
// A = 2.5 KiB + B1 = 5 KiB 2.41, A = 5 KiB 2.20, A = 5.5 KiB 2.47).
#ifndef CK_TIER_A
#define CK_TIER_A 1280
#endif
#ifndef CK_TIER_B1
#define CK_TIER_B1 1900     // (one-wave slice sizes of single-record calls: launch_single)
#endif
#ifndef CK_TIER_B2
#define CK_TIER_B2 3324
#endif
constexpr int N_TIERS = 5;
constexpr uint32_t TIER_DW[N_TIERS] = { CK_TIER_A, CK_TIER_B1, CK_TIER_B2, 9980, CK_LUT_STRIDE == 1 ? 40188u : 31996u };     // + TIER_EXTRA_DW per workgroup
constexpr uint32_t TIER_EXTRA_DW = 4 + ck::FAST_LUT_DW + ck::FAST_LUTN_DW;        // counter, decode table, N patch table
constexpr uint32_t TIER_D_DW = TIER_DW[N_TIERS - 1];
// a batch's LDS stages: A, C and the team stage (above); TIER_DW's one-wave sizes remain for single-record calls (launch_single)
constexpr int BATCH_TIERS = 3;
constexpr uint32_t BATCH_SLICE_DW[BATCH_TIERS - 1] = { CK_TIER_A, 9980 / 4 };
constexpr uint32_t TEAM_SLICE_DW = TIER_D_DW / 16;
constexpr int N_CU = 256;
// LDS dwords (or scratch dwords) the byte-wide mode needs for a record of n symbols: the largest of the three modes
// (ck::need_dw<8>), with 64 dwords of slack
inline uint64_t worst_case_dw(uint64_t n) { return 2 * ((n + 3) / 4 + 2) + (n + 31) / 32 + 1 + 64; }
constexpr uint64_t GSLICE1_DW = 1ull << 20;     // stage 1 of the global-scratch pass: up to 64 waves x 4 MiB

// Launch geometry of a batch of n records whose streaming kernel takes per_step records per workgroup and iteration (StreamC::GROUP,
// or StreamCAux::GROUP with index / strand): G virtual workgroups for the streaming kernel, the rescue pass and tier A (segment b of
// a list belongs to workgroup b; stage C and the team stage take several segments per workgroup each), cap = records one workgroup
// can see = entries of a list segment, all_cap = records per segment of the stages that walk all records of a mode-3 batch.
#ifndef CK_TAPER_DIV
#define CK_TAPER_DIV 16
#endif
struct BatchGeometry { unsigned G; uint32_t cap, all_cap, taper_seg0, taper_log2; };
inline BatchGeometry batch_geometry(uint64_t n, uint64_t per_step)
{
    const uint64_t blocks = (n + per_step - 1) / per_step;
    unsigned G = (unsigned)(blocks < (uint64_t)N_CU * CK_FAST_BPC ? blocks : (uint64_t)N_CU * CK_FAST_BPC);
    // A small batch gets more segments than the streaming kernel has workgroups with work (the others publish an empty
    // segment and leave): the stages that walk all records of a mode-3 batch deal them out all_cap at a time, and a list
    // segment is one workgroup of every stage behind -- 2000 records of 250 kb in 125 segments of 16 left half the chip idle.
    const unsigned G_small = (unsigned)(n < (uint64_t)N_CU * 16 ? n : (uint64_t)N_CU * 16);
    if (G < G_small) G = G_small;
    uint32_t cap = (uint32_t)(per_step * ((blocks + G - 1) / G));
    uint32_t all_cap = (uint32_t)((n + G - 1) / G);
    // the walking stages' segments taper off at the end (canon_core.h seg_records): three generations of G/16 segments with
    // a half, a quarter, an eighth of the records of the ones before
    uint32_t taper_seg0 = 0, taper_log2 = 0;
    if (G >= 4096 && all_cap >= (2u << CK_TAPER_GENS)) {
        while ((2u << taper_log2) <= G / CK_TAPER_DIV) ++taper_log2;
        const uint64_t gen = 1ull << taper_log2;
        taper_seg0 = G - (uint32_t)(CK_TAPER_GENS * gen);
        auto tapered = [&](uint32_t A) { uint64_t t = 0; for (int j = 1; j <= CK_TAPER_GENS; ++j) t += A >> j; return t; };
        while ((uint64_t)taper_seg0 * all_cap + gen * tapered(all_cap) < n) ++all_cap;
        if (cap < all_cap) cap = all_cap;
    }
    return { G, cap, all_cap, taper_seg0, taper_log2 };
}

}  // namespace
