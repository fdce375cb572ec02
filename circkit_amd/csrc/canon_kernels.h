// canon_kernels.h -- every __global__ kernel of the canonicalize unit: the LDS tiers, the team and global-scratch stages, the
// rescue pass, the mixed-length kernels, the streaming kernel with its count kernel, and the XXH3 passes.  The per-record and
// per-group routines are canon_core.h / canon_fast.h / canon_stream.h / canon_mixed.h / xxh3_core.h, the constants canon_config.h.
// Included once, by circkit_canon.hip, which launches them.
#pragma once
#include <hip/hip_runtime.h>

#include "canon_core.h"
#include "canon_fast.h"
#include "canon_stream.h"
#include "canon_mixed.h"
#include "xxh3_core.h"
#include "canon_config.h"
#include "canon_plan.h"

namespace {

// One wavefront per record, WPB wavefronts per workgroup, each with its own LDS slice; the last LDS dword is the
// workgroup's deferral counter.  Consumes the segmented list of the previous stage (or all records).
// T4: with the 4-bit team in the team pass.  Inlined it costs this kernel five spilled vector registers -- on its own path, but
// a kernel with a scratch allocation is ~5 us slower to dispatch, twice in EVERY batch (stages A and C; measured on config 4
// + 1 % N: 2.068 -> 2.078 ms); as a __noinline__ call it takes the kernel from 72 to 87 registers.  So two builds: the one
// without it for batches whose predecessor left the tiers next to nothing (launch_canon's tiers_idle; their few long records
// with an N in the winning window go to wave 0 alone, as before round 4), the one with it for tiers that have real work.
// (With the list entries' second flag bit the allocator's outcome for the build with it is 72 registers without spills as well --
// an outcome five lines of unrelated code can change back: the two builds stay.)
template <int WPB, bool T4 = false>
__global__ __launch_bounds__(WPB * 64, CK_TIER_WPE) void canon_kernel(ck::CanonArgs a, uint32_t nvb, uint32_t* giants)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* blk_count = lds + WPB * a.slice_dw;
    uint32_t* lut = blk_count + 4;                   // 2-bit decode table shared by the workgroup's waves
    uint32_t* lutn = lut + ck::FAST_LUT_DW;          // ...and the 'G' -> 'N' patch table of the 2-bit-with-N-mask mode
    uint32_t live = ~0u;      // bit j: this workgroup's j-th virtual workgroup has input (those from the 32nd on are walked unseen)
    if (a.list && gridDim.x < nvb) {
        // walking grid (the previous batch left the tiers next to nothing): one parallel look at this workgroup's input
        // segments; if all are empty, zero the output counts and leave -- walking them one dependent load and two barriers
        // at a time made the five idle tiers ~80 us of every batch (headline 3.74 -> 3.70 ms, same box).  If a few are not
        // (the leftovers of a mixed-length batch with N: 244 records in 32768 segments), only those are walked: stage A of
        // that batch 77 -> 70 us (what remains is its longest record in the 4-bit mode, one wave)
        const uint32_t per = a.segs_per_block, mine = (nvb - blockIdx.x + gridDim.x - 1) / gridDim.x;
        if (threadIdx.x == 0) blk_count[1] = 0;
        __syncthreads();
        uint32_t any = 0;
        for (uint32_t t = threadIdx.x; t < mine * per; t += WPB * 64) {
            const uint32_t j = t / per, sgm = (blockIdx.x + j * gridDim.x) * per + t % per;
            if (sgm < a.in_nseg && a.list_count[sgm]) { any = 1; if (j < 32) atomicOr(blk_count + 1, 1u << j); }
        }
        if (!__syncthreads_or((int)any)) {
            if (a.defer_count)
                for (uint32_t t = threadIdx.x; t < mine; t += WPB * 64) a.defer_count[blockIdx.x + t * gridDim.x] = 0;
            return;
        }
        live = ck::uniform(blk_count[1]);            // (the team pass's use of this word is behind the loop's first barrier)
    }
    ck::fast_lut_init(lut, threadIdx.x, WPB * 64);
    ck::fast_lutn_init(lutn, threadIdx.x, WPB * 64);
    const uint32_t wib = ck::uniform(threadIdx.x >> 6);
    // `nvb` virtual workgroups (one output segment each) walked by a grid that is no bigger than what keeps the chip
    // busy: on the batches where these tiers have nothing to do (the headline) one workgroup per segment was 12-28 us of
    // pure dispatch per tier
    for (uint32_t vb = blockIdx.x, j = 0; vb < nvb; vb += gridDim.x, ++j) {
        if (j < 32 && !((live >> j) & 1u)) {
            if (threadIdx.x == 0 && a.defer_count) a.defer_count[vb] = 0;
            continue;
        }
        if (threadIdx.x == 0) *blk_count = 0;
        __syncthreads();
        ck::canon_wave_loop(a, lds + wib * a.slice_dw, lut, blk_count, vb, nvb, wib, WPB, lutn);
        __syncthreads();
        if (WPB > 1) ck::team_pass(a, lds, lut, lutn, blk_count, vb, wib, WPB, true, T4);      // records too long for one wave's slice: all waves together
        if (threadIdx.x == 0 && a.defer_count) a.defer_count[vb] = *blk_count;
        if (threadIdx.x == 0 && giants && *blk_count) atomicAdd(giants, *blk_count);     // last LDS tier: tell the global-scratch kernel there is work
    }
}

// The last LDS stage: one 16-wave workgroup with the CU's whole LDS.  A record the team can take -- its 2-bit strand (with a
// few N: + the bitmask) fits 157 KiB: pure ACGT up to ~640 kb -- is canonicalized by the sixteen waves together
// (canon_core.h team mode) where the one-wave tier this replaces ran ONE wave per CU; everything else (4-bit and byte
// modes, ties, reverse-complement palindromes) is wave 0's alone with the same LDS, as before, the others waiting at the
// barrier.  a.slice_dw = a sixteenth of the LDS dwords.
// the input segments of virtual workgroup `block`, entry by entry, by all TEAM_WAVES waves of the workgroup; buf: total_dw
// dwords of LDS -- or of global scratch (canon_global_kernel): the waves of one workgroup share their CU's vector cache,
// the workgroup barriers between the team's steps order their accesses there as they do in LDS
__device__ __forceinline__ void team_stage_block(const ck::CanonArgs& a, uint32_t* buf, uint32_t total_dw, const uint32_t* lut, const uint32_t* lutn,
                                                 uint32_t* blk_count, uint32_t block, uint32_t wib)
{
    ck::CanonArgs solo = a;
    solo.slice_dw = total_dw;
    for (uint32_t sgm = block * a.segs_per_block; sgm < (block + 1) * a.segs_per_block && sgm < a.in_nseg; ++sgm) {
        const uint32_t count = a.list_count[sgm];
        const uint32_t* seg = a.list + (uint64_t)sgm * a.in_seg_cap;
        for (uint32_t i = 0; i < count; ++i) {
            const uint32_t entry = seg[i], rec = entry & ck::ENTRY_REC;
            const uint64_t len = a.offsets[rec + 1] - a.offsets[rec];
            bool done = false, no_2n = (entry & ck::ENTRY_NO_2N) != 0;
            if (len >= 48 && len < (1ull << 31)) {
                const uint32_t n = (uint32_t)len;
                int why = (entry & ck::ENTRY_NOT_ACGT) ? 1 : 3;
                if (why == 3 && ck::need_dw_strand2(n) <= total_dw) { why = ck::canon_record_team2(a, rec, buf, lut, blk_count + 1, wib, TEAM_WAVES); done = why == 0; }
                if (why == 1 && !(entry & ck::ENTRY_NO_2N) && ck::need_dw_2n(n) <= total_dw) {
                    done = ck::canon_record_team2n(a, rec, buf, lut, lutn, blk_count + 1, wib, TEAM_WAVES);
                    no_2n = true;
                }
                if (!done && why == 1 && ck::need_dw_strand4(n) <= total_dw) done = ck::canon_record_team4(a, rec, buf, blk_count + 1, wib, TEAM_WAVES) == 0;
            }
            if (!done) {
                // not the team's: wave 0 alone with the same buffer, the general routine; the others wait
                if (wib == 0) {
                    bool not_acgt = (entry & ck::ENTRY_NOT_ACGT) != 0 || no_2n;
                    if (!ck::canon_record(solo, rec, buf, lut, lutn, not_acgt, no_2n)) ck::defer_record(a, blk_count, block, rec, not_acgt, no_2n);
                }
                __syncthreads();
            }
        }
    }
}
__global__ __launch_bounds__(TEAM_WAVES * 64) void canon_team_kernel(ck::CanonArgs a, uint32_t nvb, uint32_t* giants)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t total_dw = TEAM_WAVES * a.slice_dw;
    uint32_t* blk_count = lds + total_dw;
    uint32_t* lut = blk_count + 4;
    uint32_t* lutn = lut + ck::FAST_LUT_DW;
    {
        // nothing in any of this workgroup's input segments (every ordinary batch): one parallel look, done
        const uint32_t per = a.segs_per_block, mine = blockIdx.x < nvb ? (nvb - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
        uint32_t any = 0;
        for (uint32_t t = threadIdx.x; t < mine * per; t += TEAM_WAVES * 64) {
            const uint32_t sgm = (blockIdx.x + (t / per) * gridDim.x) * per + t % per;
            if (sgm < a.in_nseg) any |= a.list_count[sgm];
        }
        if (!__syncthreads_or((int)any)) {
            for (uint32_t t = threadIdx.x; t < mine; t += TEAM_WAVES * 64) a.defer_count[blockIdx.x + t * gridDim.x] = 0;
            return;
        }
    }
    ck::fast_lut_init(lut, threadIdx.x, TEAM_WAVES * 64);
    ck::fast_lutn_init(lutn, threadIdx.x, TEAM_WAVES * 64);
    const uint32_t wib = ck::uniform(threadIdx.x >> 6);
    for (uint32_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
        if (threadIdx.x == 0) *blk_count = 0;
        __syncthreads();
        team_stage_block(a, lds, total_dw, lut, lutn, blk_count, vb, wib);
        __syncthreads();
        if (threadIdx.x == 0) {
            a.defer_count[vb] = *blk_count;
            if (giants && *blk_count) atomicAdd(giants, *blk_count);       // tell the global-scratch kernel there is work
        }
    }
}

// The end of the line: records no LDS tier can hold (2-bit beyond ~640 kb).  Same code, one wave per record, with the
// packed strands and the candidate bitmask in a slice of GLOBAL scratch instead of LDS.  The lanes of one wavefront
// hand data to each other through that memory; wave_sync()'s wavefront-scope fences are what the AMDGPU memory model
// asks for there (one wave, one L1, in-order vector memory), so canon_core.h runs unchanged.
// One launch, two phases.  Phase 1: every workgroup (one wave) takes its share of the input segments with a slice of the
// scratch; what still does not fit goes to its output segment.  Phase 2: the workgroup that finishes LAST (arrival
// ticket) takes all output segments with the WHOLE scratch -- by then nobody else uses it.  The hand-over of the
// lists between workgroups follows the agent-scope release / acquire recipe (cdna_hip_programming.md, Guideline 16):
// stores drained, release fence, ticket; the last arriver acquires before it reads.  a2 = the arguments of phase 2.
// Sixteen waves per workgroup: a record whose 2-bit strand (with a few N: + bitmask) fits the slice is the team's, as in
// canon_team_kernel, with the scratch slice in place of the LDS (a 100 Mb record: one wave took 0.29 s); the rest is wave 0's.
__global__ __launch_bounds__(TEAM_WAVES * 64) void canon_global_kernel(ck::CanonArgs a, ck::CanonArgs a2, uint32_t* scratch, uint32_t* ticket, const uint32_t* giants,
                                                                       const uint32_t* tiers_busy, uint32_t* hint_out)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *hint_out = *tiers_busy ? 2u : 1u;     // pinned host word: 1 = the tiers idled, 2 = they worked
    if (*giants == 0) return;           // nothing came out of the last LDS tier (every ordinary batch): the launch costs ~3 us, not ~12
    __shared__ uint32_t blk_count[4], lut[ck::FAST_LUT_DW], lutn[ck::FAST_LUTN_DW], last;
    ck::fast_lut_init(lut, threadIdx.x, TEAM_WAVES * 64);
    ck::fast_lutn_init(lutn, threadIdx.x, TEAM_WAVES * 64);
    const uint32_t wib = ck::uniform(threadIdx.x >> 6);
    if (threadIdx.x == 0) blk_count[0] = 0;
    __syncthreads();
    team_stage_block(a, scratch + (size_t)blockIdx.x * a.slice_dw, a.slice_dw, lut, lutn, blk_count, blockIdx.x, wib);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.defer_count[blockIdx.x] = blk_count[0];
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t arrived = atomicAdd(ticket, 1u);
        last = arrived == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            *ticket = 0;                                    // ready for the next batch
        }
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) blk_count[0] = 0;
    __syncthreads();
    team_stage_block(a2, scratch, a2.slice_dw, lut, lutn, blk_count, 0, wib);     // no output list: leftovers are counted in status[0]
}

// one record in global scratch (the host API's single-record calls)
__global__ __launch_bounds__(64) void canon_global_one_kernel(ck::CanonArgs a, uint32_t* scratch)
{
    __shared__ uint32_t blk_count, lut[ck::FAST_LUT_DW], lutn[ck::FAST_LUTN_DW];
    ck::fast_lut_init(lut, threadIdx.x, 64);
    ck::fast_lutn_init(lutn, threadIdx.x, 64);
    if (threadIdx.x == 0) blk_count = 0;
    __syncthreads();
    ck::canon_wave_loop(a, scratch, lut, &blk_count, blockIdx.x, gridDim.x, 0, 1, lutn);
}

// XXH3-64 of the listed records (the ones canon_global_kernel finished after the batch's own hash pass)
__global__ __launch_bounds__(64) void xxh3_list_kernel(const uint8_t* bytes, const uint64_t* offsets, const uint32_t* list, uint32_t count,
                                                      uint64_t* out)
{
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t r = list[i];
        const uint64_t off = offsets[r];
        const uint64_t h = ck::xxh3_64_wave(bytes + off, (uint32_t)(offsets[r + 1] - off));
        if (ck::lane_id() == 0) out[r] = h;
    }
}
// ctl: the ctx's count block (canon_plan.h CountWord: two-word records among the samples, longer ones, arrival ticket, content
// samples with a byte outside ACGT, short records) -- all zero on entry and on exit; *mode receives batch_mode_of() of the
// samples (written by the workgroup that arrives last); the counters a batch starts from zero (CTR_PASSED_ON, CTR_TIERS_BUSY,
// CTR_UNPROCESSED, the mixed ticket) are zeroed: nothing of this batch has touched them yet, nothing of the previous one is
// still running.
__global__ __launch_bounds__(1024) void stream_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n, uint32_t* ctl,
                                                            uint32_t* mode, uint32_t* counters, uint32_t hashed)
{
    __shared__ uint32_t blk[4];
    if (threadIdx.x < 4) blk[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 3) { counters[CTR_PASSED_ON] = 0; counters[CTR_TIERS_BUSY] = 0; counters[CTR_UNPROCESSED] = 0; counters[CTR_MIXED_TICKET] = 0; counters[CTR_MIXED_TICKET + 1] = 0; }      // (the mixed N builds' segment ticket is self-zeroing, zeroed here as well)
    __syncthreads();
    const uint32_t shift = count_shift(n);
    const uint64_t ns = count_samples(n);
    uint32_t two = 0, lng = 0, sht = 0; // records of 1009..2032 bases / longer ones (no build can stage their group) / short ones
    for (uint64_t j = (uint64_t)blockIdx.x * 1024 + threadIdx.x; j < ns; j += (uint64_t)gridDim.x * 1024) {
        const uint64_t i = j << shift;
        const uint64_t len = offsets[i + 1] - offsets[i];
        two += len > ck::FAST_MAX_N && len <= ck::FAST2_MAX_N;
        lng += len > ck::FAST2_MAX_N;
        sht += len <= SHORT_MAX_N;
    }
    // content samples: record k * cstep, one wave each
    const uint64_t nc = n < CONTENT_SAMPLES ? n : CONTENT_SAMPLES, cstep = n / nc;
    uint32_t bad = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * 16 + (threadIdx.x >> 6); k < nc; k += (uint64_t)gridDim.x * 16) {
        const uint64_t off = offsets[k * cstep], len = offsets[k * cstep + 1] - off;
        const uint32_t m = len < ck::FAST_MAX_N ? (uint32_t)len : ck::FAST_MAX_N, t = ck::lane_id();
        uint32_t miss = 0;
        if (m >= 16 && 16 * t < m) (void)ck::fast_pack(ck::load16(bytes + off + (16 * t + 16 <= m ? 16 * t : m - 16)), miss);
        bad += ck::ballot(miss != 0) != 0;
    }
    // one global atomic per workgroup and counter, and none for the common batch: thousands of waves adding to the
    // same two words serialise at ~10 ns each (measured: 188 us on BASELINE config 4 with one atomic per wave)
    if (ck::ballot(two | lng) != 0) {
        const uint64_t t2 = ck::wave_sum_u64(two), tl = ck::wave_sum_u64(lng);
        if (ck::lane_id() == 0 && t2) atomicAdd(&blk[0], (uint32_t)t2);
        if (ck::lane_id() == 0 && tl) atomicAdd(&blk[1], (uint32_t)tl);
    }
    if (ck::lane_id() == 0 && bad) atomicAdd(&blk[2], bad);
    if (ck::ballot(sht != 0) != 0) {                        // (none for the headline batch)
        const uint64_t ts = ck::wave_sum_u64(sht);
        if (ck::lane_id() == 0) atomicAdd(&blk[3], (uint32_t)ts);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (blk[0]) atomicAdd(ctl + CNT_TWO_WORD, blk[0]);
        if (blk[1]) atomicAdd(ctl + CNT_LONGER, blk[1]);
        if (blk[2]) atomicAdd(ctl + CNT_NOT_ACGT, blk[2]);
        if (blk[3]) atomicAdd(ctl + CNT_SHORT, blk[3]);
        // arrival ticket: the adds above are device-scope atomics (performed at the memory side, in order behind this
        // wave's earlier ones once drained), the last arriver reads the sums with atomics as well
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(ctl + CNT_TICKET, 1u) == gridDim.x - 1) {
            const uint32_t t2 = atomicExch(ctl + CNT_TWO_WORD, 0u), tl = atomicExch(ctl + CNT_LONGER, 0u), tb = atomicExch(ctl + CNT_NOT_ACGT, 0u), ts = atomicExch(ctl + CNT_SHORT, 0u);
            *mode = batch_mode_of(t2, tl, ns, tb, nc, ts, hashed != 0);
            atomicExch(ctl + CNT_TICKET, 0u);
        }
    }
}
// every kernel of a batch takes the mode from the same word (or the host's answer): bits 0..1 = stream_mode, MODE_ALPHA
__device__ __forceinline__ uint32_t batch_mode(const uint32_t* __restrict__ mode, uint32_t host_mode)
{
    return host_mode ? host_mode & 15u : *mode;         // (bit 31: MODE_GUESS, see launch_canon)
}
// Rescue pass (canon_stream.h): the streaming kernel's leftovers that are eligible by themselves, one wave per record.
// A small persistent grid walks the list segments (a batch the streaming kernel handled completely leaves them
// empty: the pass then costs a microsecond, not the dispatch of one workgroup per segment); segment s of the input
// list yields segment s of the output list, so the tiers behind keep their geometry.
// ALPHA: the build with the 4-bit register path and the prefetching loop, for batches whose mode carries MODE_ALPHA
// (builds with index / strand outputs exist only as ALPHA = false: their N-bearing records take the LDS tiers).
template <bool HASH, bool AUX, bool ALPHA>
__global__ __launch_bounds__(256) void canon_rescue_kernel(ck::CanonArgs a, const uint32_t* __restrict__ mode_word, uint32_t host_mode, uint32_t* mode_out,
                                                           uint32_t* tiers_busy)
{
    const uint32_t mode = batch_mode(mode_word, host_mode);
    if (!rescue_owns(AUX, ALPHA, mode)) return;                          // the other build has this batch, or a canon_mixed kernel
    if (blockIdx.x == 0 && threadIdx.x == 0) *mode_out = (host_mode >> 31) ? *mode_word : mode;     // for circkit_ctx_last_batch_mode() and the next batch's launch: the batch's OWN mode
    const bool all_records = AUX && (mode & 3) == 3;                    // the streaming kernel stood this batch out (only the AUX build owns such a batch)
    if (!all_records) {
        // the ordinary batch leaves this pass (next to) nothing: one parallel look at the workgroup's segments first
        const uint32_t mine = blockIdx.x < a.in_nseg ? (a.in_nseg - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
        uint32_t any = 0;
        for (uint32_t t = threadIdx.x; t < mine; t += 256) any |= a.list_count[blockIdx.x + t * gridDim.x];
        if (!__syncthreads_or((int)any)) {
            for (uint32_t t = threadIdx.x; t < mine; t += 256) a.defer_count[blockIdx.x + t * gridDim.x] = 0;
            return;
        }
    }
    __shared__ uint32_t lut[ck::FAST_LUT_DW], seg_count;
    ck::fast_lut_init(lut, threadIdx.x, 256);
    ck::RescueState<HASH, AUX> st;
    if (HASH) st.hc = ck::fast_hash_const();
    const uint32_t wib = ck::uniform(threadIdx.x >> 6);
    uint32_t passed_on = 0, walked = 0;          // (thread 0) records this workgroup hands to the tiers / segments it walked
    for (uint32_t sgm = blockIdx.x; sgm < a.in_nseg; sgm += gridDim.x) {
        if (threadIdx.x == 0) seg_count = 0;
        __syncthreads();
        ck::canon_rescue_segment<HASH, AUX, ALPHA>(a, lut, st, &seg_count, sgm, wib, 4, all_records);
        __syncthreads();
        if (threadIdx.x == 0) { a.defer_count[sgm] = seg_count; passed_on += seg_count; ++walked; }
    }
    // a hint for the NEXT batch's launch: do the LDS tiers have real work (more than one record per segment on
    // average)?  Idle tiers are launched with small grids (they walk the segments): a full-size grid that finds every
    // segment empty costs 12-17 us per tier.  Plain store, same value from whoever stores.
    if (threadIdx.x == 0 && passed_on > walked) *tiers_busy = 1;
}

// Batches of mixed lengths (mode 3: the streaming kernel stands them out): ONE kernel walks all records, four waves per
// workgroup with a stage-A slice each (canon_mixed.h).  A record of 48..1008 bases takes the register routine straight from
// memory, a longer one the LEAN LDS routine -- aligned chunks, one scan loop for both strands, the unique-minimum path only;
// the latency-bound short records and the bandwidth-bound long ones share the CUs.  Everything the lean routines do not
// decide (ties, palindromes, strangers in the alphabet, records beyond the slice) goes to segment s of the list stage A
// consumes, whose kernel carries the general routine and the team mode.  Segment s = records [s * all_seg_cap, (s + 1) *
// all_seg_cap).  NM: the build for batches whose mode carries MODE_ALPHA (N packed as G + a mask bit per symbol).
// Batches that also want the XXH3, the rotation index or the strand keep the rescue pass + stage A.
// amdgpu_num_vgpr(36): on gfx90a+ the attribute counts in the unified VGPR + AGPR file at twice the value -- 72 registers --
// and, unlike __launch_bounds__(256, 7), leaves the kernel all 102 scalar registers.  What the CU then holds is SIX of these
// workgroups, not seven: 106 SGPRs + the trap handler's 16 round to 128 of the SIMD's 800 (tools/probe_timeline.py stamps
// every workgroup: exactly 6 resident per CU; compiled for 7 waves per SIMD it has 94 SGPRs and 19 spills, for 8 it has 78 and 32).
// Measured on one box: 1.85 ms at six, 1.86 at seven, 1.98 at eight (smaller slices: more records for stage A) -- the
// kernel is bound by what a CU issues and moves per cycle, not by latency; the fewest spills win.
#ifdef CK_MIXED_TIMELINE
// Experiment builds only (tools/probe_timeline.py): start / end of every workgroup of the last mixed-length kernel on the
// 100 MHz wall clock, and the CU it ran on.
__device__ uint64_t g_timeline[3 * 65536];
#endif
template <bool NM, bool HASH>
// Segments are handed out by a TICKET (round 4): a grid of as many workgroups as the chip holds at once, each taking the next
// segment from a global counter until the segments run out -- no workgroup hand-over between segments (round 3's timeline of one
// workgroup per segment: 1450 of 1536 slots filled in the steady state), the order stays the dispatch order the tapered tail is
// built for.  ticket[0] = next segment, ticket[1] = workgroups that are through; the last one through zeroes both, so every
// launch finds them zero (a kernel that returns at its mode check never touches them).
__device__ __forceinline__ void canon_mixed_body(const ck::CanonArgs& a, const uint32_t* __restrict__ mode_word, uint32_t host_mode, uint32_t* mode_out, uint32_t* tiers_busy,
                                                 uint32_t* ticket)
{
    constexpr int WPB = mixed_wpb(NM, HASH);
    const uint32_t mode = batch_mode(mode_word, host_mode);
    if (!mixed_owns(NM, mode)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) *mode_out = (host_mode >> 31) ? *mode_word : mode;
#ifdef CK_MIXED_TIMELINE
    const uint64_t tl_start = wall_clock64();
#endif
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* blk_count = lds + WPB * a.slice_dw;
    uint32_t* lut = blk_count + 4;
    uint32_t* lutn = lut + ck::FAST_LUT_DW;                // N builds: the 'G' / 'C' -> 'N' patch tables (the output is patched in registers)
    uint32_t* htab = lutn + ck::LEAN_LUTN_DW;              // (HASH builds: the XXH3 per-pair constants)
    ck::fast_lut_init(lut, threadIdx.x, 64 * WPB);
    if (NM) ck::lean_lutn_init(lutn, threadIdx.x, 64 * WPB);
    if (HASH) ck::lean_hash_table_init(htab, threadIdx.x);
    ck::RescueState<HASH, false> st;
    if (HASH) {                                          // (only the lane's stripe secrets stay in registers: lean_hash_refill)
        st.hc.k0 = ck::xsec64(8 * (ck::lane_id() >> 2) + 16 * (ck::lane_id() & 3));
        st.hc.k1 = ck::xsec64(8 * (ck::lane_id() >> 2) + 16 * (ck::lane_id() & 3) + 8);
    }
    const uint32_t wib = ck::uniform(threadIdx.x >> 6);
    uint32_t* slice = lds + wib * a.slice_dw;
    const uint64_t payload_end = a.offsets[a.n_records];
    uint32_t passed_on = 0, walked = 0, static_sgm = blockIdx.x;
    for (;;) {
        // (ticket == nullptr: the static mapping -- workgroup b takes segments b, b + grid, ...; with one workgroup per segment
        // that is one segment each.  The pure builds keep it: handed out by ticket to a resident grid they measured 2.5 % SLOWER
        // on config 4, the N builds 2 % faster.)
        if (threadIdx.x == 0) { blk_count[0] = 0; blk_count[1] = ticket ? atomicAdd(ticket, 1u) : static_sgm; }
        static_sgm += gridDim.x;
        __syncthreads();
        const uint32_t sgm = blk_count[1];
        if (sgm >= a.in_nseg) break;                       // (every wave of every workgroup gets here: the segments run out)
        ck::canon_mixed_segment<NM, HASH>(a, slice, lut, st, blk_count, sgm, wib, WPB, payload_end, htab, lutn);
        __syncthreads();
        if (threadIdx.x == 0) { a.defer_count[sgm] = *blk_count; passed_on += *blk_count; ++walked; }
    }
    if (threadIdx.x == 0) {
        if (passed_on > walked) *tiers_busy = 1;
        if (ticket && atomicAdd(ticket + 1, 1u) == gridDim.x - 1) { atomicExch(ticket, 0u); atomicExch(ticket + 1, 0u); }
    }
#ifdef CK_MIXED_TIMELINE
    if (threadIdx.x == 0 && blockIdx.x < 65536) {
        uint32_t hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        uint32_t xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_timeline[3 * blockIdx.x] = tl_start; g_timeline[3 * blockIdx.x + 1] = wall_clock64();
        g_timeline[3 * blockIdx.x + 2] = ((uint64_t)xcc << 32) | hwid;
    }
#endif
}
#define CK_MIXED_KERNEL(NAME, NM, HASH, VGPR)                                                                                                  \
    __global__ __launch_bounds__(64 * mixed_wpb(NM, HASH)) __attribute__((amdgpu_num_vgpr(VGPR))) void NAME(ck::CanonArgs a, const uint32_t* __restrict__ mode_word, \
                                                                                     uint32_t host_mode, uint32_t* mode_out, uint32_t* tiers_busy, uint32_t* ticket) \
    {                                                                                                                                          \
        canon_mixed_body<NM, HASH>(a, mode_word, host_mode, mode_out, tiers_busy, ticket);                                                     \
    }
CK_MIXED_KERNEL(canon_mixed_kernel, false, false, 36)
CK_MIXED_KERNEL(canon_mixed_n_kernel, true, false, CK_MIXED_NM_VGPR)
CK_MIXED_KERNEL(canon_mixed_h_kernel, false, true, CK_MIXED_H_VGPR)          // + XXH3 (uniq on batches of mixed lengths)
CK_MIXED_KERNEL(canon_mixed_nh_kernel, true, true, CK_MIXED_NM_VGPR)
#undef CK_MIXED_KERNEL

// PERSIST = false: one workgroup per list segment (the build the host expects to match the batch, at full size).
// PERSIST = true: `nvb` virtual workgroups walked by a small grid -- the OTHER build, whose workgroups normally return
// at once (4-5 us instead of the ~40 us a full-size idle grid costs) and take the whole batch when the expectation was
// wrong.  Two instantiations because the loop over virtual workgroups costs the hot path scalar registers (measured:
// +2 % on the headline with one kernel for both).
// ALPHA (ROWS = 1, no index / strand outputs): the build for batches with MODE_ALPHA -- records with N or '-' take the
// 4-bit register routine inside the staged loop.  The builds without it answer for every other batch, MODE_ALPHA or not.
template <class StreamC, bool HASH, bool AUX, bool PERSIST, bool ALPHA = false>
__global__ __launch_bounds__(StreamC::WPB * 64, (StreamBuild<StreamC, HASH, AUX, ALPHA>::WPE)) void canon_stream_kernel(ck::CanonArgs a, const uint32_t* __restrict__ mode,
                                                                                                             uint32_t host_mode, uint32_t nvb)
{
    using Build = StreamBuild<StreamC, HASH, AUX, ALPHA>;
    if (!Build::owns(batch_mode(mode, host_mode))) return;                       // another build (or none) has this batch
    constexpr bool GH = Build::GH, PAIR = Build::PAIR;
    __shared__ __attribute__((aligned(16))) uint32_t lds[Build::LDS_DW];
    uint32_t* lut = lds + StreamC::NBUF * StreamC::BUF_DW;
    uint32_t* blk_count = lut + ck::FAST_LUT_DW;
    uint32_t* gh = lds + StreamC::LDS_DW;
    ck::fast_lut_init(lut, threadIdx.x, StreamC::WPB * 64);
    if (GH) ck::group_hash_init(gh + 2 * StreamC::GROUP * ck::GH_STRIDE_DW, threadIdx.x);
    if (PAIR) ck::group_hash_secret_init(gh + 2 * StreamC::GROUP * ck::GH_STRIDE_DW + ck::GH_CONST_DW, threadIdx.x);
    if (!PERSIST) {
        if (threadIdx.x == 0) *blk_count = 0;
        __syncthreads();
        ck::canon_stream_wave_loop<StreamC, HASH, AUX, GH, ALPHA>(a, lut, lds, blk_count, blockIdx.x, gridDim.x, gh);
        __syncthreads();
        if (threadIdx.x == 0) a.defer_count[blockIdx.x] = *blk_count;
        return;
    }
    for (uint32_t vb = blockIdx.x; vb < nvb; vb += gridDim.x) {
        if (threadIdx.x == 0) *blk_count = 0;
        __syncthreads();
        ck::canon_stream_wave_loop<StreamC, HASH, AUX, GH, ALPHA>(a, lut, lds, blk_count, vb, nvb, gh);
        ck::vmem_wait<0>();                              // no DMA of this virtual workgroup may land in the next one's images
        __syncthreads();
        if (threadIdx.x == 0) a.defer_count[vb] = *blk_count;
    }
}

// XXH3-64 of each record of a CSR batch, one wavefront per record (see xxh3_core.h).  With `hashed` (the flags of
// the records the streaming kernel hashed itself) a wave takes 64 records at a time, one flag per lane, and only
// visits the ones still missing -- the pass over an all-hashed batch is one byte load per record.
// view (hash-only batches): `bytes` is the INPUT payload and record r's canonical form the rotation / reverse complement of it
// that view[r] names (CanonArgs::out_view, comp = the ctx's complement table) -- nothing was written out as bytes.
__global__ __launch_bounds__(256) void xxh3_kernel(const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                                                   uint64_t* out, const uint8_t* hashed, const uint32_t* view, const uint8_t* comp)
{
    const uint32_t wave = ck::uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t n_waves = gridDim.x * 4;
    const ck::XWaveConst xk = ck::xwave_const();
    // (views: the complement table in LDS -- a reverse-strand view looks every byte up, and the short records' lanes each their own)
    __shared__ uint8_t comp_lds[256];
    if (view) { comp_lds[threadIdx.x] = comp[threadIdx.x]; __syncthreads(); comp = comp_lds; }
    if (!hashed) {
        for (uint64_t r = wave; r < n_records; r += n_waves) {
            const uint64_t off = offsets[r];
            const uint64_t h = ck::xxh3_64_wave(bytes + off, (uint32_t)(offsets[r + 1] - off), xk);
            if (ck::lane_id() == 0) out[r] = h;
        }
        return;
    }
    // A wave looks at `span` consecutive records at a time: 512 (8 flags per lane) when the batch is big enough to keep every wave
    // busy that way, fewer -- a multiple of 64 -- for smaller batches: with 512 a million-record batch of mixed lengths whose
    // hashes are all still to do (the N build of the mixed kernel) kept a quarter of the waves busy, 2.85 ms for 4.3 GB.
    const uint64_t per_wave = (n_records + n_waves - 1) / n_waves;
    const uint32_t span = per_wave >= 512 ? 512u : (per_wave <= 64 ? 64u : (uint32_t)((per_wave + 63) / 64) * 64u);
    // up to 512 flags per look (8 per lane, one 8-byte load: the flag array is 8-byte aligned and padded): an all-hashed batch of
    // 10M records is 2-3 dependent loads per wave instead of 19 (28 -> ~8 us per batch)
    for (uint64_t big = (uint64_t)wave * span; big < n_records; big += (uint64_t)n_waves * span) {
      const uint64_t f0 = big + 8 * ck::lane_id();
      uint64_t flags8 = ~0ull;
      if (f0 < n_records && 8 * ck::lane_id() < span) {
          flags8 = *reinterpret_cast<const uint64_t*>(hashed + f0);
          if (n_records - f0 < 8) flags8 |= ~0ull << (8 * (n_records - f0));       // bytes past the last record
      }
      // a zero byte = a record still to hash
      if (ck::ballot(((flags8 - 0x0101010101010101ull) & ~flags8 & 0x8080808080808080ull) != 0) == 0) continue;
      for (uint64_t base = big; base < big + span && base < n_records; base += 64) {
        const uint64_t mine = base + ck::lane_id();
        const bool need = mine < n_records && !hashed[mine];
        uint64_t todo = ck::ballot(need);
        if (!todo) continue;
        // the chunk's offsets in one coalesced load (lane L: record base + L), handed out by v_readlane: no dependent
        // round trip in front of every record
        const uint64_t my_off = need ? offsets[mine] : 0;
        const uint32_t my_len = need ? (uint32_t)(offsets[mine + 1] - my_off) : 0u;
        // XXH3's short-input classes (<= 240 bytes) are ONE scalar recipe (xxh3_short): every lane hashes its own record instead of
        // the whole wave hashing one after the other -- a batch of short reads (20M x 200 b, none of whose hashes the kernels
        // in front fuse) took 58 ms with bytes, 89 ms from views; ~60 times fewer instructions this way
        const bool mine_short = need && my_len <= 240u;
        const uint64_t shorts = ck::ballot(mine_short);
        if (shorts) {
            if (mine_short) {
                const uint8_t* p = bytes + my_off;
                uint64_t h;
                if (view) {
                    const uint32_t v = view[mine], rot = v & 0x7FFFFFFFu;
                    h = ck::xxh3_short(ck::XView{ p, my_len, rot < my_len ? rot : 0u, (v >> 31) != 0, comp }, my_len);
                } else h = ck::xxh3_short(ck::XPlain{ p }, my_len);
                out[mine] = h;
            }
            todo &= ~shorts;
        }
        while (todo) {
            const uint32_t l = (uint32_t)ck::ffs64(todo);
            todo &= todo - 1;
            const uint64_t off = ((uint64_t)ck::readlane((uint32_t)(my_off >> 32), l) << 32) | ck::readlane((uint32_t)my_off, l);
            const uint32_t len = ck::readlane(my_len, l);
            const uint64_t h = view ? ck::xxh3_64_wave_view(bytes + off, len, view[base + l], comp, xk) : ck::xxh3_64_wave(bytes + off, len, xk);
            if (ck::lane_id() == 0) out[base + l] = h;
        }
      }
    }
}

}  // namespace
