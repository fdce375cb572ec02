// circkit_canon.hip -- canonicalize: the host side of a batch (launch_canon, one function per stage, the front stages by canon_plan.h's plan), of a single record
// (launch_single) and of a host-buffer batch in parts (host_batch), and the C ABI of include/circkit.h that runs or reports on
// that work.  The kernels are canon_kernels.h, the constants and the batch geometry canon_config.h; the ctx (circkit_hip.hip)
// is seen with its fields, through ck_ctx_impl.h: the canonicalize state is allocated with it.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>

#include "../../include/circkit.h"
#include "canon_kernels.h"
#include "ck_ctx_impl.h"

namespace {

int ensure_lists(circkit_ctx* c, uint64_t entries, uint64_t segs)
{
    int rc;
    for (auto& list : c->d_lists)           // (all of one size: a list that is large enough already stays)
        if ((rc = list.grow(c, entries))) return rc;
    if (segs > c->seg_alloc) {
        c->seg_alloc = 0;
        if ((rc = c->d_seg_counts.grow(c, (N_TIERS + 1) * segs))) return rc;
        c->seg_alloc = segs;
    }
    return CIRCKIT_OK;
}

// What one stage of a batch hands to the next: the kernel arguments as the stage before left them, and the segments and the
// capacity of the list the next stage consumes.  The rest is fixed for the batch.
struct Batch {
    ck::CanonArgs a;
    unsigned nseg;
    uint32_t seg_cap;
    unsigned G;                     // virtual workgroups of the streaming kernel, the rescue pass and tier A (batch_geometry)
    uint32_t host_mode, kmode;      // the mode the host has seen or guessed (0: the device decides) / what the kernels get (+ bit 31: guessed)
    bool aux;                       // the rotation index, the strand or the forward-only variant is wanted
};
inline const uint32_t* mode_word(const circkit_ctx* c) { return c->d_counters + CTR_MODE; }

// The kernels of the front builds, entry for entry of FRONT_BUILDS (canon_plan.h).  A streaming build has two: [1] one workgroup
// per list segment, for the batch it is expected to own; [0] its PERSIST twin, which walks the G virtual workgroups with a small
// grid, returns at once when the batch is not its own and takes the whole batch when the expectation was wrong.
using StreamFn = void (*)(ck::CanonArgs, const uint32_t*, uint32_t, uint32_t);
using RescueFn = void (*)(ck::CanonArgs, const uint32_t*, uint32_t, uint32_t*, uint32_t*);
using MixedFn = void (*)(ck::CanonArgs, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*);
struct FrontKernel { StreamFn stream[2]; RescueFn rescue; MixedFn mixed; };
const FrontKernel FRONT_KERNELS[N_FRONT_BUILDS] = {
#define CK_X(id, CFG, HASH, AUX, ALPHA) { { canon_stream_kernel<CFG, HASH, AUX, true, ALPHA>, canon_stream_kernel<CFG, HASH, AUX, false, ALPHA> }, nullptr, nullptr },
    CK_STREAM_BUILDS(CK_X)
#undef CK_X
#define CK_X(id, HASH, AUX, ALPHA) { {}, canon_rescue_kernel<HASH, AUX, ALPHA>, nullptr },
    CK_RESCUE_BUILDS(CK_X)
#undef CK_X
#define CK_X(id, KERNEL, NM, HASH) { {}, nullptr, KERNEL },
    CK_MIXED_BUILDS(CK_X)
#undef CK_X
};

// Stages 1 to 3, the front of a batch: the streaming kernel over every record (what it cannot take goes down the LDS tiers), the
// rescue pass over its leftovers, segment for segment into the next list, and -- mode 3 -- a mixed-length kernel over every
// record in its place (same lists, same segments).  Which builds are launched, and with which grid, is canon_front_plan's.
void stage_front(circkit_ctx* c, Batch& b, bool device_decides)
{
    ck::CanonArgs& a = b.a;
    const bool hash = a.out_hash != nullptr;
    if (device_decides) {
        const uint64_t ns = count_samples(a.n_records);
        const unsigned cgrid = (unsigned)((ns + 1023) / 1024 < 128 ? (ns + 1023) / 1024 : 128);
        hipLaunchKernelGGL(stream_count_kernel, dim3(cgrid), dim3(1024), 0, c->stream, a.bytes, a.offsets, a.n_records, c->d_counters + CTR_COUNT, c->d_counters + CTR_MODE, (uint32_t*)c->d_counters, (hash && !b.aux) ? 1u : 0u);
    }
    // (the mode of whichever earlier batch last reported, straight from pinned host memory: a hint for the grid sizes, nothing else)
    const FrontPlan plan = canon_front_plan(b.aux, hash, b.host_mode, c->h_mode[HM_MODE], b.G, b.nseg);
    for (int i = 0; i < plan.n; ++i) {
        const FrontLaunch& e = plan.e[i];
        const FrontBuild& fb = FRONT_BUILDS[e.build];
        const FrontKernel& k = FRONT_KERNELS[e.build];
        const dim3 grid(e.grid), block(fb.block);
        if (fb.stage == FRONT_STREAM) { a.list = nullptr; a.list_count = nullptr; }
        else {
            a.list = c->d_lists[0]; a.list_count = c->d_seg_counts;
            a.in_nseg = b.nseg; a.in_seg_cap = b.seg_cap; a.segs_per_block = 1;
        }
        const int out = fb.stage == FRONT_STREAM ? 0 : 1;
        a.defer_list = c->d_lists[out]; a.defer_count = c->d_seg_counts + out * c->seg_alloc; a.out_seg_cap = b.seg_cap;
        a.slice_dw = fb.slice_dw;
        // (the batch's mode goes straight into pinned host memory, c->d_mode: no copy-back, no event)
        if (fb.stage == FRONT_STREAM) hipLaunchKernelGGL(k.stream[e.full], grid, block, 0, c->stream, a, mode_word(c), b.kmode, b.G);
        else if (fb.stage == FRONT_RESCUE) hipLaunchKernelGGL(k.rescue, grid, block, 0, c->stream, a, mode_word(c), b.kmode, c->d_mode + HM_MODE, c->d_counters + CTR_TIERS_BUSY);
        else hipLaunchKernelGGL(k.mixed, grid, block, fb.lds, c->stream, a, mode_word(c), b.kmode, c->d_mode + HM_MODE, c->d_counters + CTR_TIERS_BUSY,
                                fb.alpha ? c->d_counters + CTR_MIXED_TICKET : (uint32_t*)nullptr);
    }
}

#ifdef CK_DEBUG_DUMP
// experiment builds only (tools/build_variant.sh -DCK_DEBUG_DUMP, tools/leftover_hist.py): what the front kernels handed to stage A
void dump_stage_a_input(circkit_ctx* c, const Batch& b)
{
    const unsigned nseg = b.nseg;
    const uint32_t seg_cap = b.seg_cap;
    const uint64_t n = b.a.n_records;
    const uint64_t* d_offsets = b.a.offsets;
    (void)hipStreamSynchronize(c->stream);
    std::vector<uint32_t> cnt(nseg);
    (void)hipMemcpy(cnt.data(), c->d_seg_counts + c->seg_alloc, nseg * 4, hipMemcpyDeviceToHost);
    uint64_t total = 0; unsigned shown = 0;
    if (getenv("CK_DUMP_HIST")) {       // length histogram of the deferred records (powers of two), flagged / not
        std::vector<uint32_t> ents((size_t)nseg * seg_cap);
        (void)hipMemcpy(ents.data(), c->d_lists[1], ents.size() * 4, hipMemcpyDeviceToHost);
        std::vector<uint64_t> offs(n + 1);
        (void)hipMemcpy(offs.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost);
        uint64_t hist[2][32] = {}, bytes[2] = {};
        for (unsigned sg = 0; sg < nseg; ++sg)
            for (uint32_t k = 0; k < cnt[sg]; ++k) {
                const uint32_t e = ents[(size_t)sg * seg_cap + k]; const uint64_t len = offs[(e & ck::ENTRY_REC) + 1] - offs[e & ck::ENTRY_REC];
                hist[e >> 31][63 - __builtin_clzll(len | 1)]++; bytes[e >> 31] += len;
            }
        for (int f = 0; f < 2; ++f) { fprintf(stderr, "[dump] flag %d (%llu bytes):", f, (unsigned long long)bytes[f]); for (int b2 = 0; b2 < 32; ++b2) if (hist[f][b2]) fprintf(stderr, " 2^%d:%llu", b2, (unsigned long long)hist[f][b2]); fprintf(stderr, "\n"); }
    }
    for (unsigned sg = 0; sg < nseg; ++sg) {
        total += cnt[sg];
        for (uint32_t k = 0; k < cnt[sg] && shown < 12; ++k, ++shown) {
            uint32_t e = 0; uint64_t o[2];
            (void)hipMemcpy(&e, c->d_lists[1] + (uint64_t)sg * seg_cap + k, 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(o, d_offsets + (e & ck::ENTRY_REC), 16, hipMemcpyDeviceToHost);
            fprintf(stderr, "[dump] seg %u entry %u: rec %u flag %u len %llu\n", sg, k, e & ck::ENTRY_REC, e >> 31, (unsigned long long)(o[1] - o[0]));
        }
    }
    fprintf(stderr, "[dump] stage A input: %llu records in %u segments\n", (unsigned long long)total, nseg);
}
#endif

// Stage 4: the LDS tiers A, C and the team stage, each consuming the list of the stage before.
void stage_tiers(circkit_ctx* c, Batch& b)
{
    ck::CanonArgs& a = b.a;
    const bool tiers_idle = c->h_mode[HM_TIERS] == 1;       // the previous batch's tiers found (next to) nothing: small grids for this one
    // (What the idle tiers cost live, measured by not launching them: 82 us of the 3.70 ms headline step, 116 us of uniq's
    // 5.26; with the parallel look at the counts in canon_kernel ~40 us remain -- five dependent launches.)
    for (int t = 0; t < BATCH_TIERS; ++t) {
        const unsigned nseg = b.nseg;
        const uint32_t seg_cap = b.seg_cap;
        const bool last = t == BATCH_TIERS - 1;
        // stage C merges four segments per workgroup when there are plenty (its workgroups are four to a CU); a small batch
        // keeps one segment per workgroup -- 4000 records of 120 kb are 250 segments: 63 workgroups would leave the chip idle
        const unsigned spb = t == 0 ? 1 : (last ? (nseg + N_CU - 1) / N_CU : (nseg >= 16u * N_CU ? 4 : 1));
        const unsigned grid = (nseg + spb - 1) / spb;
        a.list = c->d_lists[t + 1]; a.list_count = c->d_seg_counts + (uint64_t)(t + 1) * c->seg_alloc;
        a.in_nseg = nseg; a.in_seg_cap = seg_cap; a.segs_per_block = spb;
        // the last tier's leftovers go into the first list (long consumed by now): the global-scratch stages pick them up
        a.defer_list = last ? c->d_lists[0] : c->d_lists[t + 2];
        a.defer_count = last ? c->d_seg_counts : c->d_seg_counts + (uint64_t)(t + 2) * c->seg_alloc;
        a.out_seg_cap = spb * seg_cap;
        a.slice_dw = last ? TEAM_SLICE_DW : BATCH_SLICE_DW[t];
        // `grid` virtual workgroups; launched: a few times what is resident at once (dispatch order balances the rest)
        const unsigned bpc = tiers_idle ? CK_TIER_BPC_IDLE : CK_TIER_BPC;
        const unsigned launched = grid < (unsigned)N_CU * bpc ? grid : (unsigned)N_CU * bpc;
        if (last) hipLaunchKernelGGL(canon_team_kernel, dim3(launched), dim3(TEAM_WAVES * 64), (TEAM_WAVES * TEAM_SLICE_DW + TIER_EXTRA_DW) * 4, c->stream, a, grid, c->d_counters + CTR_PASSED_ON);
        else hipLaunchKernelGGL((tiers_idle ? canon_kernel<4, false> : canon_kernel<4, true>), dim3(launched), dim3(256), (4 * a.slice_dw + TIER_EXTRA_DW) * 4, c->stream, a, grid, (uint32_t*)nullptr);
        b.nseg = grid;
        b.seg_cap = spb * seg_cap;
    }
}

// Stage 5: records no LDS tier can hold (2-bit beyond ~640 kb, byte-mode beyond ~70 kb): the same code, one wave per
// record, with a slice of the global scratch in place of the LDS slice -- one more launch.  Phase 1: up to 64
// waves x 4 MiB (2-bit records up to ~16.7 Mb); phase 2 (the last workgroup to finish): one wave with the whole
// scratch (256 MiB by default: 2-bit up to ~1 Gb -- ~700 Mb if the minimal key ties --, bytes up to ~126 MB;
// circkit_ctx_set_long_record_scratch).
// Beyond: counted in status[0].
void stage_global(circkit_ctx* c, Batch& b)
{
    ck::CanonArgs& a = b.a;
    const unsigned nseg = b.nseg;
    const uint32_t seg_cap = b.seg_cap;
    const uint64_t cap_dw = c->d_gscratch.cap / 4;
    const uint64_t slice1 = cap_dw < GSLICE1_DW ? cap_dw : GSLICE1_DW;
    const unsigned max_w1 = (unsigned)(cap_dw / slice1 < 64 ? cap_dw / slice1 : 64);
    const unsigned spb1 = (nseg + max_w1 - 1) / max_w1, w1 = (nseg + spb1 - 1) / spb1;
    a.list = c->d_lists[0]; a.list_count = c->d_seg_counts;
    a.in_nseg = nseg; a.in_seg_cap = seg_cap; a.segs_per_block = spb1;
    a.defer_list = c->d_lists[1]; a.defer_count = c->d_seg_counts + c->seg_alloc; a.out_seg_cap = spb1 * seg_cap;
    a.slice_dw = (uint32_t)slice1;
    ck::CanonArgs a2 = a;
    a2.list = c->d_lists[1]; a2.list_count = c->d_seg_counts + c->seg_alloc;
    a2.in_nseg = w1; a2.in_seg_cap = spb1 * seg_cap; a2.segs_per_block = w1;
    a2.defer_list = nullptr; a2.defer_count = nullptr; a2.out_seg_cap = 0;
    a2.slice_dw = (uint32_t)(cap_dw < 0xFFFFFFFFull ? cap_dw : 0xFFFFFFFFull);
    hipLaunchKernelGGL(canon_global_kernel, dim3(w1), dim3(TEAM_WAVES * 64), 0, c->stream, a, a2, (uint32_t*)c->d_gscratch.p, c->d_counters + CTR_GLOBAL_TICKET,
                       (const uint32_t*)(c->d_counters + CTR_PASSED_ON), (const uint32_t*)(c->d_counters + CTR_TIERS_BUSY), c->d_mode + HM_TIERS);
}

// Stage 6: the XXH3 of the records whose hash was not fused: from their canonical bytes, or (hash-only batch) from the input
// through their views.
void stage_leftover_xxh3(circkit_ctx* c, const Batch& b)
{
    const ck::CanonArgs& a = b.a;
    if (!a.out_hash) return;
    const uint8_t* src = a.out_view ? a.bytes : a.out_bytes;
    hipLaunchKernelGGL(xxh3_kernel, dim3(b.G < 2048u ? b.G : 2048u), dim3(256), 0, c->stream, src, a.offsets, a.n_records, a.out_hash, (const uint8_t*)c->d_hashed,
                       (const uint32_t*)a.out_view, a.out_view ? (const uint8_t*)c->d_comp : nullptr);
}

// Enqueues one batch: every kernel, nothing else -- no host-side follow-up is needed once the stream has run them
// (records beyond the on-chip tiers included: the last two stages take them in a global-memory scratch).
// host_mode: 1 / 2 / 3 when the host has seen the offsets (stream_mode), 0 = the device decides.
int launch_canon(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint8_t* d_out,
                 uint32_t* d_idx, uint8_t* d_strand, uint64_t* d_hash, uint32_t flags, uint32_t host_mode = 0, bool keep_status = false)
{
    if (n >= (1ull << 30)) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records must be < 2^30");      // (list entries: 30 bits of record index)
    CK_HIP(c, hipSetDevice(c->device));
    if (n == 0) { c->timed = false; return CIRCKIT_OK; }
    // MODE_GUESS.  Every mode computes the same results -- the mode only says which builds are the fast ones for the batch's
    // lengths and alphabet.  A device batch whose mode the host does not know used to launch every build (the ones the
    // device-side decision does not name return at once): eleven idle kernels per batch, ~5 us each, 3-4 % of a 1.8 ms
    // batch.  Now the mode the last batches REPORTED (the pinned word the device writes, read here without waiting) is taken as
    // this batch's mode, exactly as if the host had seen the offsets: only that mode's kernels are launched.  The count
    // kernel still runs and the kernels report ITS answer (bit 31 of the mode argument), so the guess follows the data: a
    // batch of another kind runs correctly on the wrong builds (as slow as round 2's general path at worst), the launch after
    // the one that sees the new report decides on the device again, the one after that guesses the new mode.
    // CIRCKIT_NO_MODE_GUESS=1: every batch decides on the device, as before.
    const bool device_decides = host_mode == 0;
    uint32_t guess_flag = 0;
    if (device_decides) {
        static const bool no_guess = getenv("CIRCKIT_NO_MODE_GUESS") != nullptr;
        const uint32_t seen = c->h_mode[HM_MODE] & 15u;
        if (!no_guess && (seen & 3u) && seen == c->mode_seen) { host_mode = seen; guess_flag = 0x80000000u; }
        c->mode_seen = seen;
        static const bool dbg = getenv("CIRCKIT_DEBUG_MODE_GUESS") != nullptr;
        if (dbg) fprintf(stderr, "[mode guess] n=%llu report=%u -> %s\n", (unsigned long long)n, seen, guess_flag ? "guessed" : "decided on the device");
    }
    const bool aux = d_idx || d_strand || (flags & ck::CK_FLAG_FWD_ONLY);
    const BatchGeometry g = batch_geometry(n, aux ? StreamCAux::GROUP : StreamC::GROUP);    // (per_step: records a workgroup takes per iteration)
    // + 1024 segments of slack: a stage that merges k segments per workgroup addresses up to k - 1 segments past the end
    int rc = ensure_lists(c, (uint64_t)g.G * g.cap + 1024ull * g.cap, g.G < 256u ? 256u : g.G);
    if (rc) return rc;
    if (!c->d_gscratch && (rc = c->d_gscratch.grow(c, c->gscratch_default))) return rc;
    uint32_t* view = nullptr;
    if (d_hash && !d_out) {
        // hash-only (uniq without --canonicalize, src/uniq.rs:55-60): no canonical bytes are written anywhere.  A record
        // whose hash is not fused leaves its canonical form as a view of the input -- strand + rotation, one u32 in a ctx
        // array sized by n (known here: no look at the device, no synchronisation) -- and the xxh3 pass hashes that view.
        if (n > c->d_view.cap && (rc = c->d_view.grow(c, n + n / 8 + 64))) return rc;
        view = c->d_view;
    }
    if (d_hash) {
        if (n > c->d_hashed.cap && (rc = c->d_hashed.grow(c, n + n / 8 + 64))) return rc;
        CK_HIP(c, hipMemsetAsync(c->d_hashed, 0, n, c->stream));
    }
    // d_counters (canon_plan.h CounterWord): a device-side decision zeroes the words a batch starts from in its count kernel, the
    // host-side one with a memset.
    // (keep_status: a later part of a host batch -- CTR_UNPROCESSED, the records nothing could take, adds up over the parts)
    if (!device_decides) CK_HIP(c, hipMemsetAsync(c->d_counters, 0, (keep_status ? CTR_UNPROCESSED : CTR_ZEROED_PER_BATCH) * sizeof(uint32_t), c->stream));
    CK_HIP(c, hipEventRecord(c->ev0, c->stream));
    Batch b{};
    ck::CanonArgs& a = b.a;
    a.bytes = d_bytes; a.offsets = d_offsets; a.n_records = n;
    a.out_bytes = d_out; a.out_index = d_idx; a.out_strand = d_strand; a.out_hash = d_hash; a.hashed = c->d_hashed; a.out_view = view;
    a.comp_lut = c->d_comp; a.status = c->d_counters + CTR_UNPROCESSED; a.flags = flags;
    a.all_seg_cap = g.all_cap; a.taper_seg0 = g.taper_seg0; a.taper_log2 = g.taper_log2;
    b.nseg = g.G; b.seg_cap = g.cap; b.G = g.G;
    b.host_mode = host_mode; b.kmode = host_mode | guess_flag; b.aux = aux;
    stage_front(c, b, device_decides);
#ifdef CK_DEBUG_DUMP
    dump_stage_a_input(c, b);
#endif
    stage_tiers(c, b);
    stage_global(c, b);
    stage_leftover_xxh3(c, b);
    CK_HIP(c, hipEventRecord(c->ev1, c->stream));
    CK_HIP(c, hipGetLastError());
    c->timed = true;
    return CIRCKIT_OK;
}

// One record through the host API (the lib-crate mirrors circkit_lmsr_index / _lmsr / _canonicalize): a single launch
// of the general per-record kernel with the smallest slice that holds the record in any mode, instead of the batch
// pipeline's dozen launches.
int launch_single(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t len, uint8_t* d_out, uint32_t* d_idx,
                  uint8_t* d_strand, uint64_t* d_hash, uint32_t flags)
{
    ck::CanonArgs a{};
    a.bytes = d_bytes; a.offsets = d_offsets; a.n_records = 1;
    a.out_bytes = d_out; a.out_index = d_idx; a.out_strand = d_strand; a.out_hash = nullptr; a.hashed = nullptr;
    a.comp_lut = c->d_comp; a.status = c->d_counters + CTR_UNPROCESSED; a.flags = flags;
    CK_HIP(c, hipMemsetAsync(c->d_counters + CTR_UNPROCESSED, 0, sizeof(uint32_t), c->stream));
    const uint64_t need = worst_case_dw(len);
    int t = 0;
    while (t < N_TIERS && TIER_DW[t] < need) ++t;
    if (t < N_TIERS) {
        a.slice_dw = TIER_DW[t];
        hipLaunchKernelGGL(canon_kernel<1>, dim3(1), dim3(64), (TIER_DW[t] + TIER_EXTRA_DW) * 4, c->stream, a, 1u, (uint32_t*)nullptr);
    } else {
        int rc = c->d_gscratch.grow(c, need * 4);
        if (rc) return rc;
        a.slice_dw = (uint32_t)(need < 0xFFFFFFFFull ? need : 0xFFFFFFFFull);
        hipLaunchKernelGGL(canon_global_one_kernel, dim3(1), dim3(64), 0, c->stream, a, (uint32_t*)c->d_gscratch.p);
    }
    if (d_hash) hipLaunchKernelGGL(xxh3_kernel, dim3(1), dim3(256), 0, c->stream, d_out, d_offsets, (uint64_t)1, d_hash, (const uint8_t*)nullptr, (const uint32_t*)nullptr, (const uint8_t*)nullptr);
    CK_HIP(c, hipGetLastError());
    c->timed = false;
    return CIRCKIT_OK;
}

// (the buffer grown last answers for its group: after a failed allocation it has not grown, and the group is grown again)
int ensure_staging(circkit_ctx* c, uint64_t bytes, uint64_t recs)
{
    int rc;
    if (bytes + 64 > c->d_out.cap) {
        const uint64_t nb = bytes + bytes / 8 + 4096;
        if ((rc = c->d_in.grow(c, nb)) || (rc = c->d_out.grow(c, nb))) return rc;
    }
    if (recs + 1 > c->d_hash.cap) {
        const uint64_t nr = recs + recs / 8 + 1024;
        if ((rc = c->d_off.grow(c, nr)) || (rc = c->d_idx.grow(c, nr)) || (rc = c->d_strand.grow(c, nr)) || (rc = c->d_hash.grow(c, nr))) return rc;
    }
    return CIRCKIT_OK;
}

int host_batch_enqueue(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* out,
                       uint32_t* idx, uint8_t* strand, uint64_t* hash, uint32_t flags);
// Every error exit of the host-buffer path drains the ctx's streams before it returns: copies of earlier parts into the caller's
// `out` and out of the ctx's page-locked staging may still be in flight when a later part fails, and the caller is free to
// release its buffers the moment the call is back.
int host_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* out,
               uint32_t* idx, uint8_t* strand, uint64_t* hash, uint32_t flags)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    const int rc = host_batch_enqueue(c, bytes, offsets, n, out, idx, strand, hash, flags);
    if (rc != CIRCKIT_OK) {
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->s_out) (void)hipStreamSynchronize(c->s_out);
    }
    return rc;
}
int host_batch_enqueue(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint8_t* out,
                       uint32_t* idx, uint8_t* strand, uint64_t* hash, uint32_t flags)
{
    if (n && (!offsets || offsets[0] != 0)) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    if (n == 0) return CIRCKIT_OK;
    const uint64_t total = offsets[n];
    if (total && !bytes) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "bytes is NULL");
    CK_HIP(c, hipSetDevice(c->device));
    int rc = ensure_staging(c, total, n);
    if (rc) return rc;
    const bool need_bytes = out || hash;
    static const bool dbg_t = getenv("CIRCKIT_DEBUG_TIMING") != nullptr;
    auto dbg_t0 = std::chrono::steady_clock::now();
    auto dbg_lap = [&](const char* what) {
        if (!dbg_t) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "  host_batch %-18s %.3f ms\n", what, std::chrono::duration<double>(now - dbg_t0).count() * 1e3);
        dbg_t0 = now;
    };
    uint64_t two_word = 0, longer = 0, shorter = 0, max_len = 0;   // the host has the offsets: it picks the streaming kernel's build
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets decrease at record %llu", (unsigned long long)i);
        const uint64_t len = offsets[i + 1] - offsets[i];
        two_word += len > ck::FAST_MAX_N && len <= ck::FAST2_MAX_N;
        longer += len > ck::FAST2_MAX_N;
        shorter += len <= SHORT_MAX_N;
        max_len = len > max_len ? len : max_len;
    }
    if (max_len >> 31) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "a record of 2^31 symbols or more (cyclic positions are 32-bit)");
    if (n == 1 && (max_len + 15) / 16 + 2 <= TIER_DW[0]) {     // (a longer record is worth the batch pipeline: its team stages)
        if (total) CK_HIP(c, hipMemcpyAsync(c->d_in, bytes, total, hipMemcpyHostToDevice, c->stream));
        CK_HIP(c, hipMemcpyAsync(c->d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
        rc = launch_single(c, c->d_in, c->d_off, max_len, need_bytes ? c->d_out : nullptr, idx ? c->d_idx : nullptr,
                           strand ? c->d_strand : nullptr, hash ? c->d_hash : nullptr, flags);
        if (rc) return rc;
        if (out && total) CK_HIP(c, hipMemcpyAsync(out, c->d_out, total, hipMemcpyDeviceToHost, c->stream));
        if (idx) CK_HIP(c, hipMemcpyAsync(idx, c->d_idx, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (strand) CK_HIP(c, hipMemcpyAsync(strand, c->d_strand, n, hipMemcpyDeviceToHost, c->stream));
        if (hash) CK_HIP(c, hipMemcpyAsync(hash, c->d_hash, n * 8, hipMemcpyDeviceToHost, c->stream));
        uint32_t unprocessed = 0;
        CK_HIP(c, hipMemcpyAsync(&unprocessed, c->d_counters + CTR_UNPROCESSED, 4, hipMemcpyDeviceToHost, c->stream));
        CK_HIP(c, hipStreamSynchronize(c->stream));
        if (unprocessed) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "%u record(s) could not be processed", unprocessed);
        return CIRCKIT_OK;
    }
    // ...sizes the global scratch for the longest record, whatever mode it turns out to need
    // (never less than the device entry points' size: on a fresh ctx a scratch sized for this batch alone would stay the ctx's --
    // launch_canon allocates the default only when there is none -- and a later device batch would find its long records refused)
    if (worst_case_dw(max_len) > TIER_D_DW) {
        const uint64_t want = worst_case_dw(max_len) * 4;
        if ((rc = c->d_gscratch.grow(c, want < c->gscratch_default ? c->gscratch_default : want))) return rc;
    }
    // The batch goes through the device in PARTS of >= 16 MB (up to sixteen): part k + 1 is copied in while part k - 1 is copied
    // out on a stream of the ctx's own; with page-locked buffers (circkit_host_alloc) the two directions of the link work at
    // the same time.  One part = the round-2 behaviour: in, compute, out, one after the other
    // (1 GB of 1 kb records: 37.9 ms per call, 53 GB/s for both directions together).
    dbg_lap("offset scan");
    // (measured, tools/probe_host_batch.py: 64 MB in four parts 1.93 ms; 256 MB in eight 6.48 ms, in sixteen 6.84; 1 GB in eight
    // 25.2 ms, in sixteen 24.3, in thirty-two 24.4-24.8: up to eight parts of 16 MB and more, beyond 512 MB sixteen of 64 MB)
    int parts = (int)(total / (16ull << 20));
    parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
    if (total > (512ull << 20)) { parts = (int)(total / (64ull << 20)); parts = parts > 16 ? 16 : parts; }
    parts = parts > circkit_ctx::MAX_PARTS ? circkit_ctx::MAX_PARTS : parts;
    if ((uint64_t)parts > n) parts = (int)n;
    if (getenv("CIRCKIT_HOST_BATCH_PARTS")) { const int p = atoi(getenv("CIRCKIT_HOST_BATCH_PARTS")); if (p >= 1 && p <= circkit_ctx::MAX_PARTS && (uint64_t)p <= n) parts = p; }
    // The copy-in rides the ctx stream itself, part k + 1 queued behind part k's kernels (a few hundred microseconds next to the
    // milliseconds of a part's copy); the copy-out has a stream of the ctx's own, at a priority of its own (the runtime keeps
    // a separate set of hardware queues per priority: no queue shared with the ctx stream or any default-priority stream).
    // With a plain copy-in and a plain copy-out stream -- round 3's first arrangement, dropped since -- the two directions of a
    // call overlapped or took turns (1 GB: 24.8 or 38-40 ms) depending on how many streams the process had made before.  In this
    // arrangement only a process that runs straight behind one that has just released tens of GB of device memory is slow: for
    // some seconds the copy engines are busy with the driver's handling of that memory (tools/probe_after_big_process.sh);
    // bench.py's end-to-end leg waits it out.  A copy kernel that stores across the link instead of the DMA engine: 28 ms.
    if (!c->s_out) {
        int prio_least = 0, prio_greatest = 0;
        CK_HIP(c, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
        CK_HIP(c, hipStreamCreateWithPriority(&c->s_out, hipStreamNonBlocking, prio_greatest));
        CK_HIP(c, hipEventCreateWithFlags(&c->ev_head, hipEventDisableTiming));
        for (hipEvent_t& e : c->ev_done) CK_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    // part boundaries: record indices, cut where the payload passes k / parts of its bytes
    uint64_t cut[circkit_ctx::MAX_PARTS + 1];
    cut[0] = 0; cut[parts] = n;
    for (int k = 1; k < parts; ++k) {
        const uint64_t want = total / parts * k;
        uint64_t lo = cut[k - 1] + 1, hi = n - (parts - k);               // keep every part non-empty
        if (lo > hi) lo = hi;
        while (lo < hi) { const uint64_t mid = (lo + hi) / 2; if (offsets[mid] < want) lo = mid + 1; else hi = mid; }
        cut[k] = lo;
    }
    // whatever the caller has queued on the ctx stream comes first; the offsets go with the first part
    CK_HIP(c, hipEventRecord(c->ev_head, c->stream));
    // (through a page-locked copy of them: from the caller's pageable array the runtime stages the copy and the call blocks
    // until it is through -- 0.9 ms of a 64 MB batch's 4.2)
    // The per-record outputs (hash, index, strand: 13 bytes a record) come back the same way: into page-locked staging part by
    // part, to the caller's arrays once at the end -- a copy-out to pageable memory would hold up every part behind it
    // (uniq on 1M x 1 kb: 38.6 ms per call with the hashes going straight to a pageable array, 23.7 without hashes).
    constexpr uint64_t PER_REC = 8 + 8 + 4 + 1;           // offset, hash, index, strand
    if ((n + 1) * PER_REC > c->h_stage.cap && (rc = c->h_stage.grow(c, (n + 1 + (n + 1) / 8 + 1024) * PER_REC))) return rc;
    const uint64_t st_recs = c->h_stage.cap / PER_REC;
    uint64_t* const st_off = (uint64_t*)c->h_stage.p;
    uint64_t* const st_hash = st_off + st_recs;
    uint32_t* const st_idx = (uint32_t*)(st_hash + st_recs);
    uint8_t* const st_strand = (uint8_t*)(st_idx + st_recs);
    memcpy(st_off, offsets, (n + 1) * 8);
    CK_HIP(c, hipMemcpyAsync(c->d_off, st_off, (n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    auto copy_in = [&](int k) -> int {
        const uint64_t b0 = offsets[cut[k]], b1 = offsets[cut[k + 1]];
        if (b1 > b0) CK_HIP(c, hipMemcpyAsync(c->d_in + b0, bytes + b0, b1 - b0, hipMemcpyHostToDevice, c->stream));
        return CIRCKIT_OK;
    };
    if ((rc = copy_in(0))) return rc;
    dbg_lap("enqueue copy-in");
    // ...and, while the first part is on its way, samples the content like stream_count_kernel does (a byte outside ACGT in
    // the first 1008 of a sampled record) -- on an eighth of that kernel's sample: the rule asks whether a sixteenth of the
    // records hold such a byte, and either answer gives the same output (it picks the faster build).  Up front and over all
    // 4096 samples this loop was 1.5-2.4 ms of EVERY call, more than the 16 MB batch it was deciding about took to cross the link.
    const uint64_t nc = n < CONTENT_SAMPLES / 8 ? n : CONTENT_SAMPLES / 8, cstep = n / nc;
    uint64_t bad = 0;
    {
        static const struct Acgt { uint8_t no[256]; Acgt() { memset(no, 1, sizeof no); no['A'] = no['C'] = no['G'] = no['T'] = 0; } } acgt;
        for (uint64_t k = 0; k < nc; ++k) {
            const uint64_t o = offsets[k * cstep], len = offsets[k * cstep + 1] - o, m = len < ck::FAST_MAX_N ? len : ck::FAST_MAX_N;
            uint32_t b = 0;
            for (uint64_t i = 0; i < m; ++i) b |= acgt.no[bytes[o + i]];
            bad += b;
        }
    }
    const uint32_t host_mode = batch_mode_of(two_word, longer, n, bad, nc, shorter, hash != nullptr && !idx && !strand && !(flags & ck::CK_FLAG_FWD_ONLY));
    dbg_lap("content sample");
    volatile uint32_t* unprocessed = c->h_mode + HM_UNPROCESSED;          // (pinned)
    for (int k = 0; k < parts; ++k) {
        const uint64_t r0 = cut[k], nk = cut[k + 1] - r0, b0 = offsets[r0], b1 = offsets[cut[k + 1]];
        rc = launch_canon(c, c->d_in, c->d_off + r0, nk, need_bytes ? c->d_out : nullptr, idx ? c->d_idx + r0 : nullptr,
                          strand ? c->d_strand + r0 : nullptr, hash ? c->d_hash + r0 : nullptr, flags, host_mode, k > 0);
        if (rc) return rc;                                  // (host_batch drains the streams)
        CK_HIP(c, hipEventRecord(c->ev_done[k], c->stream));
        CK_HIP(c, hipStreamWaitEvent(c->s_out, c->ev_done[k], 0));
        if (k + 1 < parts && (rc = copy_in(k + 1))) return rc;
        if (out && b1 > b0) CK_HIP(c, hipMemcpyAsync(out + b0, c->d_out + b0, b1 - b0, hipMemcpyDeviceToHost, c->s_out));
        if (idx) CK_HIP(c, hipMemcpyAsync(st_idx + r0, c->d_idx + r0, nk * 4, hipMemcpyDeviceToHost, c->s_out));
        if (strand) CK_HIP(c, hipMemcpyAsync(st_strand + r0, c->d_strand + r0, nk, hipMemcpyDeviceToHost, c->s_out));
        if (hash) CK_HIP(c, hipMemcpyAsync(st_hash + r0, c->d_hash + r0, nk * 8, hipMemcpyDeviceToHost, c->s_out));
    }
    // the count of records nothing could take, added up over the parts (only part 0's launch zeroes it): read once, behind the
    // last part -- a copy of it per part made every part's kernels wait for the copy-out two parts back
    unprocessed[0] = 0;
    CK_HIP(c, hipMemcpyAsync((void*)unprocessed, c->d_counters + CTR_UNPROCESSED, 4, hipMemcpyDeviceToHost, c->s_out));
    dbg_lap("enqueue parts");
    CK_HIP(c, hipStreamSynchronize(c->s_out));
    dbg_lap("sync copy-out");
    CK_HIP(c, hipStreamSynchronize(c->stream));
    dbg_lap("sync stream");
    if (idx) memcpy(idx, st_idx, n * 4);
    if (strand) memcpy(strand, st_strand, n);
    if (hash) memcpy(hash, st_hash, n * 8);
    const uint32_t lost = unprocessed[0];
    if (lost) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "%u record(s) could not be processed", lost);
    return CIRCKIT_OK;
}

}  // namespace

// the last step of circkit_ctx_create (ck_ctx_impl.h): the one-wave tier and the team stage take more LDS than the default limit
int ck_canon_init(circkit_ctx* c)
{
    CK_HIP(c, hipFuncSetAttribute((const void*)canon_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)((TIER_D_DW + TIER_EXTRA_DW) * 4)));
    CK_HIP(c, hipFuncSetAttribute((const void*)canon_team_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)((TEAM_WAVES * TEAM_SLICE_DW + TIER_EXTRA_DW) * 4)));
    return CIRCKIT_OK;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int circkit_ctx_last_kernel_ms(circkit_ctx* c, float* ms)
{
    if (!c || !ms) return CIRCKIT_ERR_INVALID_ARG;
    if (!c->timed) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "no timed batch yet");
    CK_HIP(c, hipEventSynchronize(c->ev1));
    CK_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return CIRCKIT_OK;
}

int circkit_ctx_batch_status(circkit_ctx* c, uint32_t* n_unprocessed)
{
    if (!c || !n_unprocessed) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    *n_unprocessed = 0;
    CK_HIP(c, hipMemcpyAsync(n_unprocessed, c->d_counters + CTR_UNPROCESSED, 4, hipMemcpyDeviceToHost, c->stream));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    if (*n_unprocessed)
        return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "%u record(s) were not processed: longer than the long-record scratch (%llu MiB, "
                    "circkit_ctx_set_long_record_scratch) or than 2^31 symbols", *n_unprocessed, (unsigned long long)(c->d_gscratch.cap >> 20));
    return CIRCKIT_OK;
}

int circkit_ctx_set_long_record_scratch(circkit_ctx* c, uint64_t bytes)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    if (bytes < (1ull << 20)) bytes = 1ull << 20;
    c->gscratch_default = bytes;
    CK_HIP(c, hipStreamSynchronize(c->stream));        // a batch in flight may be using the old one
    return c->d_gscratch.grow(c, bytes);
}

int circkit_ctx_last_batch_mode(circkit_ctx* c, uint32_t* mode)
{
    if (!c || !mode) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    *mode = c->h_mode[HM_MODE] & 3;
    return CIRCKIT_OK;
}

int circkit_canonicalize_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                      uint64_t n, uint8_t* d_out, uint32_t* d_idx, uint8_t* d_strand,
                                      uint64_t* d_hash)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n && !d_offsets) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_offsets is NULL");
    return launch_canon(c, d_bytes, d_offsets, n, d_out, d_idx, d_strand, d_hash, 0);
}

int circkit_lmsr_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                              uint8_t* d_out, uint32_t* d_idx)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n && !d_offsets) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_offsets is NULL");
    return launch_canon(c, d_bytes, d_offsets, n, d_out, d_idx, nullptr, nullptr, ck::CK_FLAG_FWD_ONLY);
}

int circkit_canonicalize_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                               uint8_t* out, uint32_t* idx, uint8_t* strand, uint64_t* hash)
{
    return host_batch(c, bytes, offsets, n, out, idx, strand, hash, 0);
}

static int check_ascii(circkit_ctx* c, const uint8_t* s, size_t n)
{
    if (n && !s) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "s is NULL");
    if (n >= (1ull << 31)) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "record too long");
    for (size_t i = 0; i < n; ++i)
        if (s[i] & 0x80) return ck_fail(c, CIRCKIT_ERR_NOT_ASCII, "non-ASCII byte at %zu (the reference panics on non-UTF-8 / indexes by char)", i);
    return CIRCKIT_OK;
}

int circkit_lmsr_index(circkit_ctx* c, const uint8_t* s, size_t n, size_t* out_index)
{
    if (!c || !out_index) return CIRCKIT_ERR_INVALID_ARG;
    int rc = check_ascii(c, s, n);
    if (rc) return rc;
    *out_index = 0;
    if (n == 0) return CIRCKIT_OK;                      // lib/src/canonicalize.rs:8-11: res stays 0
    uint64_t off[2] = { 0, (uint64_t)n };
    uint32_t idx = 0;
    rc = host_batch(c, s, off, 1, nullptr, &idx, nullptr, nullptr, ck::CK_FLAG_FWD_ONLY);
    *out_index = idx;
    return rc;
}

int circkit_lmsr(circkit_ctx* c, const uint8_t* s, size_t n, uint8_t* out)
{
    if (!c || (n && !out)) return CIRCKIT_ERR_INVALID_ARG;
    int rc = check_ascii(c, s, n);
    if (rc || n == 0) return rc;
    uint64_t off[2] = { 0, (uint64_t)n };
    return host_batch(c, s, off, 1, out, nullptr, nullptr, nullptr, ck::CK_FLAG_FWD_ONLY);
}

int circkit_canonicalize(circkit_ctx* c, const uint8_t* s, size_t n, uint8_t* out)
{
    if (!c || (n && !out)) return CIRCKIT_ERR_INVALID_ARG;
    int rc = check_ascii(c, s, n);
    if (rc || n == 0) return rc;
    uint64_t off[2] = { 0, (uint64_t)n };
    return host_batch(c, s, off, 1, out, nullptr, nullptr, nullptr, 0);
}

int circkit_xxh3_64(circkit_ctx* c, const uint8_t* s, size_t n, uint64_t* out_hash)
{
    if (!c || !out_hash || (n && !s)) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    int rc = ensure_staging(c, n, 1);
    if (rc) return rc;
    uint64_t off[2] = { 0, (uint64_t)n };
    if (n) CK_HIP(c, hipMemcpyAsync(c->d_in, s, n, hipMemcpyHostToDevice, c->stream));
    CK_HIP(c, hipMemcpyAsync(c->d_off, off, 16, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(xxh3_kernel, dim3(1), dim3(256), 0, c->stream, c->d_in, c->d_off, (uint64_t)1, c->d_hash, (const uint8_t*)nullptr, (const uint32_t*)nullptr, (const uint8_t*)nullptr);
    CK_HIP(c, hipMemcpyAsync(out_hash, c->d_hash, 8, hipMemcpyDeviceToHost, c->stream));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    return CIRCKIT_OK;
}

int circkit_xxh3_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                              uint64_t* d_hash)
{
    if (!c || (n && (!d_offsets || !d_hash))) return CIRCKIT_ERR_INVALID_ARG;
    if (n == 0) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(c->device));
    const uint64_t blocks = (n + 3) / 4;
    const unsigned grid = (unsigned)(blocks < (uint64_t)N_CU * 8 ? blocks : (uint64_t)N_CU * 8);
    hipLaunchKernelGGL(xxh3_kernel, dim3(grid), dim3(256), 0, c->stream, d_bytes, d_offsets, n, d_hash, (const uint8_t*)nullptr, (const uint32_t*)nullptr, (const uint8_t*)nullptr);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

#ifdef CK_MIXED_TIMELINE
int circkit_debug_timeline(circkit_ctx* c, uint64_t* host, uint32_t n_wg)
{
    if (!c || !host || n_wg > 65536) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    CK_HIP(c, hipMemcpyFromSymbol(host, HIP_SYMBOL(g_timeline), (size_t)n_wg * 24));
    return CIRCKIT_OK;
}
#endif

#ifdef CK_DEBUG_POISON
// Test build only (tests/poison.py; not in include/circkit.h): records of all batches since ctx creation whose staged chunk was
// read before its DMA had landed (canon_stream.h stream_poison).  Synchronizes.
int circkit_debug_poison_count(circkit_ctx* c, uint32_t* n)
{
    if (!c || !n) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    CK_HIP(c, hipMemcpy(n, c->d_counters + CTR_POISON, 4, hipMemcpyDeviceToHost));
    return CIRCKIT_OK;
}
#endif

}  // extern "C"
