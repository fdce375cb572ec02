// circkit_monomerize.hip -- `circkit monomerize` on the GPU: the entry points of include/circkit.h's monomerize section.
//
// monomerize_kernel: one wave per record runs ck_mono::record_end (monomerize.h) and lane 0 stores the record's end index
// (or CIRCKIT_MONOMER_NONE).  Nothing else is written: the monomer is a prefix of the input.  The record is read from
// global memory whatever its length (16-byte loads, contiguous across the wave); a 1 kb record is one scan step, a long one
// is walked by the same wave step by step.  Records of 2^32 symbols or more are not processed (NONE); the host form refuses
// the batch with CIRCKIT_ERR_TOO_LONG.
//
// Compact (the writer closure on the device, monomer_compact.h): compact_decide_kernel applies the writer's filters, one lane
// per record; three scan kernels (ck_scan.h's bodies over PairAdd) turn (written, written length) into each written record's
// slot and byte offset and the two totals; compact_gather_kernel packs the monomers, by output bytes.  All five are enqueued back to back: the totals stay in
// ctx-owned device memory, which is why the gather runs a fixed grid that strides over however many tiles there turn out to be.
// Everything behind the decide kernel knows a record only by its word w[i], and is open to the other units through
// ck_compact_launch.h: circkit_uniq_compact.hip fills w from uniq's first_seen and has the dropped records listed as well.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"            // the ctx lives in circkit_hip.hip; this file sees it through this header
#include "ck_compact_launch.h"
#include "ck_scan.h"
#include "monomerize.h"
#include "monomer_compact.h"


namespace {

constexpr int MONO_WG = 256, MONO_WAVES = MONO_WG / 64;
constexpr uint64_t MONO_MAX_GRID = 1u << 20;      // waves stride over the records beyond this many workgroups

__global__ __launch_bounds__(MONO_WG) void monomerize_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                             uint64_t n, ck_mono::Params P, uint32_t* __restrict__ out_end)
{
    const uint64_t stride = (uint64_t)gridDim.x * MONO_WAVES;
    for (uint64_t i = (uint64_t)blockIdx.x * MONO_WAVES + ck::wave_in_block(); i < n; i += stride) {
        const uint64_t o = ck::uniform64(offsets[i]), L = ck::uniform64(offsets[i + 1]) - o;
        uint32_t r = ck_mono::NONE;
        if (L <= 0xFFFFFFFFull) r = ck_mono::record_end(bytes + o, (uint32_t)L, P);
        if (ck::lane_id() == 0) out_end[i] = r;
    }
}


// ---- compact: decide, scan, gather ------------------------------------------------------------------------------------
constexpr int COMPACT_WG = 256;                       // decide: one lane per record
constexpr int CSCAN_WG = 256, CSCAN_ITEMS = 8, CSCAN_TILE = CSCAN_WG * CSCAN_ITEMS;      // records per scan tile: 2048
constexpr uint32_t COMPACT_MAX_GRID = 1u << 20;       // decide strides over the records beyond this many workgroups
constexpr uint32_t GATHER_GRID = 2048;                // workgroups of the gather: 8 per CU, striding over the output tiles
enum { T_RECORDS = CK_COMPACT_RECORDS, T_BYTES = CK_COMPACT_BYTES, T_OVERLAP = CK_COMPACT_OVERLAP, T_WORDS = CK_COMPACT_WORDS };      // the totals of a compact, in device memory

__global__ __launch_bounds__(COMPACT_WG) void compact_decide_kernel(const uint64_t* __restrict__ offsets, uint64_t n,
                                                                    const uint32_t* __restrict__ end, const uint64_t* __restrict__ full_len,
                                                                    ck_compact::Filter F, uint64_t* __restrict__ w, uint32_t* __restrict__ kept_end)
{
    const uint64_t stride = (uint64_t)gridDim.x * COMPACT_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * COMPACT_WG + threadIdx.x; i < n; i += stride) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        uint32_t kept;
        w[i] = ck_compact::decide(len, full_len ? full_len[i] : len, end[i], F, &kept);
        if (kept_end) kept_end[i] = kept;
    }
}

struct Pair { uint64_t cnt, bytes; };                 // written records, written bytes
__device__ inline Pair pair_of(uint64_t w) { return Pair{ w >> 63, w & ~ck_compact::WRITTEN }; }
struct PairAdd {                                      // the scan's operation (ck_scan.h): both sums at once
    typedef Pair T;
    CK_DEV T identity() { return Pair{ 0, 0 }; }
    CK_DEV T combine(T earlier, T later) { return Pair{ earlier.cnt + later.cnt, earlier.bytes + later.bytes }; }
};

__global__ __launch_bounds__(CSCAN_WG) void compact_tile_sums_kernel(const uint64_t* __restrict__ w, uint64_t n, Pair* __restrict__ sums)
{
    __shared__ Pair lds[CSCAN_WG];
    const Pair total = ck_scan::tile_sum<CSCAN_WG, CSCAN_ITEMS, PairAdd>(threadIdx.x, blockIdx.x, w, n, [](uint64_t x) { return pair_of(x); }, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the tile sums become exclusive, CSCAN_WG of them at a time; then the totals, out_offsets[0], and the refusal of
// an output buffer that overlaps the input payload (its owed room: as many bytes as the payload), after which nothing is written.
__global__ __launch_bounds__(CSCAN_WG) void compact_scan_sums_kernel(Pair* __restrict__ sums, uint64_t n_tiles, const uint8_t* bytes,
                                                                     const uint64_t* __restrict__ offsets, uint64_t n, const uint8_t* out,
                                                                     uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ totals)
{
    __shared__ Pair lds[CSCAN_WG];
    const Pair carry = ck_scan::sums_exclusive<CSCAN_WG, PairAdd>(threadIdx.x, sums, n_tiles, lds);
    if (threadIdx.x == 0) {
        bool overlap = false;
        if (n) {
            const uint64_t p0 = offsets[0], p1 = offsets[n];
            const uintptr_t in_lo = (uintptr_t)bytes + p0, in_hi = (uintptr_t)bytes + p1, out_lo = (uintptr_t)out, out_hi = out_lo + (p1 - p0);
            overlap = p1 > p0 && out_lo < in_hi && in_lo < out_hi;
        }
        totals[T_RECORDS] = overlap ? 0 : carry.cnt;
        totals[T_BYTES] = overlap ? 0 : carry.bytes;
        totals[T_OVERLAP] = overlap ? 1 : 0;
        if (out_offsets) out_offsets[0] = 0;
    }
}

// written record i goes to slot j: out_offsets[j + 1] = where it ends, out_src[j] = i, src_start[j] = where it starts in the input.
// A dropped record i goes to slot i - (the written records before it) of the dropped list, which the running j already is:
// dup_src[slot] = i, dup_first[slot] = dup_val[i], each where the pointer is given.
__global__ __launch_bounds__(CSCAN_WG) void compact_apply_kernel(const uint64_t* __restrict__ w, uint64_t n, const Pair* __restrict__ sums,
                                                                 const uint64_t* __restrict__ totals, const uint64_t* __restrict__ offsets,
                                                                 uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ out_src,
                                                                 uint64_t* __restrict__ src_start, uint64_t* __restrict__ dup_src,
                                                                 uint64_t* __restrict__ dup_first, const uint64_t* __restrict__ dup_val)
{
    __shared__ Pair lds[CSCAN_WG];
    if (totals[T_OVERLAP]) return;                    // the same for the whole grid
    const uint64_t t0 = (uint64_t)blockIdx.x * CSCAN_TILE + (uint64_t)threadIdx.x * CSCAN_ITEMS;
    uint64_t loc[CSCAN_ITEMS];
    const Pair base = ck_scan::tile_base<CSCAN_WG, CSCAN_ITEMS, PairAdd>(threadIdx.x, blockIdx.x, w, n, [](uint64_t x) { return pair_of(x); }, sums, lds, loc);
    uint64_t j = base.cnt, at = base.bytes;
    for (int k = 0; k < CSCAN_ITEMS; ++k) {
        if (!(loc[k] & ck_compact::WRITTEN)) {
            if (t0 + k < n) {
                const uint64_t slot = t0 + k - j;
                if (dup_src) dup_src[slot] = t0 + k;
                if (dup_first) dup_first[slot] = dup_val[t0 + k];
            }
            continue;
        }
        at += loc[k] & ~ck_compact::WRITTEN;
        out_offsets[j + 1] = at;
        out_src[j] = t0 + k;
        src_start[j] = offsets[t0 + k];
        ++j;
    }
}

__global__ __launch_bounds__(64 * ck_compact::GATHER_WAVES) void compact_gather_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                                                        uint64_t n, const uint64_t* __restrict__ out_offsets,
                                                                                        const uint64_t* __restrict__ src_start,
                                                                                        const uint64_t* __restrict__ totals, uint8_t* __restrict__ out)
{
    ck_compact::Gather G;
    G.bytes = bytes;
    G.p0 = offsets[0]; G.p1 = offsets[n];
    G.out_offsets = out_offsets; G.src_start = src_start;
    G.m = totals[T_RECORDS]; G.B = totals[T_BYTES];
    G.out = out;
    if (G.B == 0) return;
    const uint64_t n_gran = (((uint64_t)(uintptr_t)out & 15u) + G.B + 15) / 16;
    const uint64_t n_tiles = (n_gran + ck_compact::TILE_GRANULES - 1) / ck_compact::TILE_GRANULES;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ck_compact::gather_tile(G, t);
}

struct MonoState {                   // host-buffer form staging
    ck_csr_buf in;
    ck_buf<uint32_t> d_end;
    // compact: scan scratch, the totals on the device and their pinned copy
    ck_buf<uint64_t> d_w, d_src_start;
    ck_buf<Pair> d_sums;
    ck_totals totals;                // [T_WORDS], made at the first compact
    bool host_last = false;          // the last compact was the host form: its totals are host_totals
    uint64_t host_totals[T_WORDS] = { 0, 0, 0 };
    // compact, host-buffer form staging
    ck_buf<uint8_t> d_out;
    ck_buf<uint64_t> d_out_off, d_out_src, d_full;
    ck_buf<uint32_t> d_kept;
};

MonoState* state(circkit_ctx* c) { return ck_unit_state<MonoState>(c, CK_UNIT_MONOMERIZE); }

// the walk both host forms make behind their params: the unit takes records below 2^32 symbols
int check_offsets(circkit_ctx* c, const uint64_t* offsets, uint64_t n)
{
    uint64_t at = 0;
    const ck_csr_fault fault = ck_csr_walk(offsets, n, 1ull << 32, &at);
    if (fault == CK_CSR_DECREASE) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (fault) return ck_ctx_fail(c, CIRCKIT_ERR_TOO_LONG, "a record of 2^32 symbols or more");
    return CIRCKIT_OK;
}

// MonomerizerBuilder::validate (lib/src/monomerize.rs:20-40) + the CLI's range check of the identity (src/monomerize.rs:40-44)
int make_params(circkit_ctx* c, const circkit_monomerize_params* p, ck_mono::Params* P)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null params");
    if (p->seed_len < 1 || p->seed_len > 63)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "Seed length must be at least 1 and at most 63");
    if (p->use_identity && !(p->min_identity >= 0.0 && p->min_identity <= 1.0))      // NaN fails both comparisons
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "min_identity must be between 0.0 and 1.0");
    P->overlap_dist = p->overlap_dist;
    P->min_identity = p->use_identity ? p->min_identity : 0.0;
    P->seed_len = p->seed_len;
    P->use_identity = p->use_identity ? 1 : 0;
    P->sensitive = p->sensitive ? 1 : 0;
    return CIRCKIT_OK;
}

int launch(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const ck_mono::Params& P, uint32_t* d_end)
{
    if (n == 0) return CIRCKIT_OK;
    uint64_t grid = (n + MONO_WAVES - 1) / MONO_WAVES;
    if (grid > MONO_MAX_GRID) grid = MONO_MAX_GRID;
    hipLaunchKernelGGL(monomerize_kernel, dim3((uint32_t)grid), dim3(MONO_WG), 0, ck_ctx_stream(c), d_bytes, d_offsets, n, P, d_end);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// the five kernels of a compact and the copy of its totals, on the ctx stream; nothing waits
int launch_compact(circkit_ctx* c, MonoState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_end,
                   const uint64_t* d_full_len, const circkit_monomer_filter* f, uint8_t* d_out_bytes, uint64_t* d_out_offsets,
                   uint64_t* d_out_src, uint32_t* d_kept_end)
{
    ck_compact::Filter F;
    F.min_length = f->min_length; F.max_length = f->max_length; F.min_overlap = f->min_overlap;
    F.min_overlap_percent = f->min_overlap_percent;
    F.use_percent = f->use_min_overlap_percent ? 1 : 0;
    F.keep_all = f->keep_all ? 1 : 0;
    uint64_t* d_w;
    int rc;
    if ((rc = ck_compact_reserve(c, n, &d_w))) return rc;
    if (n) {
        uint64_t grid = (n + COMPACT_WG - 1) / COMPACT_WG;
        if (grid > COMPACT_MAX_GRID) grid = COMPACT_MAX_GRID;
        hipLaunchKernelGGL(compact_decide_kernel, dim3((uint32_t)grid), dim3(COMPACT_WG), 0, ck_ctx_stream(c), d_offsets, n, d_end, d_full_len, F,
                           d_w, d_kept_end);
    }
    if ((rc = ck_compact_launch(c, &S->totals, d_bytes, d_offsets, n, d_out_bytes, d_out_offsets, d_out_src, nullptr, nullptr, nullptr))) return rc;
    S->host_last = false;
    return CIRCKIT_OK;
}

int check_totals(circkit_ctx* c, const uint64_t* t)
{
    if (t[T_OVERLAP]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_bytes overlaps the input payload: nothing was written");
    return CIRCKIT_OK;
}

}  // namespace

// ---- ck_compact_launch.h: the scan, apply and gather for whoever filled w ----------------------------------------------------
int ck_compact_reserve(circkit_ctx* c, uint64_t n, uint64_t** d_w)
{
    MonoState* S = state(c);
    const uint64_t tiles = (n + CSCAN_TILE - 1) / CSCAN_TILE;
    int rc;
    if ((rc = S->d_w.grow(c, n))) return rc;
    if ((rc = S->d_sums.grow(c, tiles))) return rc;
    if ((rc = S->d_src_start.grow(c, n))) return rc;
    *d_w = S->d_w;
    return CIRCKIT_OK;
}

int ck_compact_launch(circkit_ctx* c, ck_totals* T, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src, uint64_t* d_dup_src, uint64_t* d_dup_first,
                      const uint64_t* d_dup_val)
{
    MonoState* S = state(c);                          // (sized by ck_compact_reserve for this n)
    int rc;
    if ((rc = ck_totals_make(c, T, T_WORDS))) return rc;
    const uint64_t tiles = (n + CSCAN_TILE - 1) / CSCAN_TILE;
    hipStream_t st = ck_ctx_stream(c);
    if (n) hipLaunchKernelGGL(compact_tile_sums_kernel, dim3((uint32_t)tiles), dim3(CSCAN_WG), 0, st, (const uint64_t*)S->d_w, n, S->d_sums);
    hipLaunchKernelGGL(compact_scan_sums_kernel, dim3(1), dim3(CSCAN_WG), 0, st, S->d_sums, tiles, d_bytes, d_offsets, n,
                       (const uint8_t*)d_out_bytes, d_out_offsets, T->d);
    if (n) {
        hipLaunchKernelGGL(compact_apply_kernel, dim3((uint32_t)tiles), dim3(CSCAN_WG), 0, st, (const uint64_t*)S->d_w, n, (const Pair*)S->d_sums,
                           (const uint64_t*)T->d, d_offsets, d_out_offsets, d_out_src, S->d_src_start, d_dup_src, d_dup_first, d_dup_val);
        hipLaunchKernelGGL(compact_gather_kernel, dim3(GATHER_GRID), dim3(64 * ck_compact::GATHER_WAVES), 0, st, d_bytes, d_offsets, n,
                           (const uint64_t*)d_out_offsets, (const uint64_t*)S->d_src_start, (const uint64_t*)T->d, d_out_bytes);
    }
    CK_HIP(c, hipGetLastError());
    return ck_totals_fetch(c, T, T_WORDS);
}

extern "C" {

int circkit_monomerize_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                                    const circkit_monomerize_params* params, uint32_t* d_end)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!d_offsets || (n && (!d_bytes || !d_end))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    ck_mono::Params P;
    int rc = make_params(c, params, &P);
    if (rc) return rc;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    return launch(c, d_bytes, d_offsets, n, P, d_end);
}

int circkit_monomerize_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n,
                             const circkit_monomerize_params* params, uint32_t* end)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!offsets || (n && !end) || (n && !bytes && offsets[n] > offsets[0])) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    ck_mono::Params P;
    int rc = make_params(c, params, &P);
    if (rc) return rc;
    if ((rc = check_offsets(c, offsets, n))) return rc;
    if (n == 0) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    MonoState* S = state(c);
    if ((rc = S->in.upload(c, bytes, offsets, n))) return rc;
    if ((rc = S->d_end.grow(c, n))) return rc;
    if ((rc = launch(c, S->in.bytes, S->in.off, n, P, S->d_end))) return rc;
    if ((rc = S->d_end.download(c, end, n))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    return CIRCKIT_OK;
}

int circkit_monomer_end_index(circkit_ctx* c, const uint8_t* s, size_t n, const circkit_monomerize_params* params,
                              size_t* end, int* found)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!s && n) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null sequence");
    const uint64_t offs[2] = { 0, (uint64_t)n };
    uint32_t e = CIRCKIT_MONOMER_NONE;
    const int rc = circkit_monomerize_batch(c, s, offs, 1, params, &e);
    if (rc) return rc;
    if (found) *found = e != CIRCKIT_MONOMER_NONE;
    if (end) *end = e != CIRCKIT_MONOMER_NONE ? (size_t)e : n;
    return CIRCKIT_OK;
}

int circkit_monomers_compact_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_end,
                                    const uint64_t* d_full_len, const circkit_monomer_filter* filter, uint8_t* d_out_bytes,
                                    uint64_t* d_out_offsets, uint64_t* d_out_src, uint32_t* d_kept_end)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!filter) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null filter");
    if (n && (!d_bytes || !d_offsets || !d_end || !d_out_bytes || !d_out_offsets || !d_out_src))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    return launch_compact(c, state(c), d_bytes, d_offsets, n, d_end, d_full_len, filter, d_out_bytes, d_out_offsets, d_out_src, d_kept_end);
}

int circkit_monomers_status(circkit_ctx* c, uint64_t* n_kept, uint64_t* kept_bytes)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    MonoState* S = state(c);
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->host_last ? S->host_totals : S->totals.h ? S->totals.h : none;
    if (n_kept) *n_kept = t[T_RECORDS];
    if (kept_bytes) *kept_bytes = t[T_BYTES];
    return check_totals(c, t);
}

int circkit_monomers_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const circkit_monomerize_params* params,
                           const circkit_monomer_filter* filter, const uint64_t* full_len, uint8_t* out_bytes, uint64_t* out_offsets,
                           uint64_t* out_src, uint32_t* kept_end, uint64_t* n_kept)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!filter) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null filter");
    if (!offsets || !out_offsets || (n && (!out_src || (offsets[n] > offsets[0] && (!bytes || !out_bytes)))))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    ck_mono::Params P;
    int rc = make_params(c, params, &P);
    if (rc) return rc;
    if ((rc = check_offsets(c, offsets, n))) return rc;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    MonoState* S = state(c);
    out_offsets[0] = 0;
    if (n_kept) *n_kept = 0;
    S->host_last = true;
    S->host_totals[T_RECORDS] = S->host_totals[T_BYTES] = S->host_totals[T_OVERLAP] = 0;
    if (n == 0) return CIRCKIT_OK;
    const uint64_t nb = offsets[n];
    if ((rc = S->in.upload(c, bytes, offsets, n))) return rc;
    if ((rc = S->d_end.grow(c, n))) return rc;
    if ((rc = S->d_out.grow(c, nb))) return rc;
    if ((rc = S->d_out_off.grow(c, n + 1))) return rc;
    if ((rc = S->d_out_src.grow(c, n))) return rc;
    if ((rc = S->d_kept.grow(c, n))) return rc;
    if (full_len && (rc = S->d_full.upload(c, full_len, n))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = launch(c, S->in.bytes, S->in.off, n, P, S->d_end))) return rc;
    if ((rc = launch_compact(c, S, S->in.bytes, S->in.off, n, S->d_end, full_len ? S->d_full.p : nullptr, filter, S->d_out, S->d_out_off,
                             S->d_out_src, S->d_kept))) return rc;
    CK_HIP(c, hipStreamSynchronize(st));
    S->host_last = true;
    for (int k = 0; k < T_WORDS; ++k) S->host_totals[k] = S->totals.h[k];
    if ((rc = check_totals(c, S->host_totals))) return rc;
    const uint64_t m = S->host_totals[T_RECORDS], B = S->host_totals[T_BYTES];
    if ((rc = S->d_out_off.download(c, out_offsets, m + 1))) return rc;
    if ((rc = S->d_out_src.download(c, out_src, m))) return rc;
    if ((rc = S->d_kept.download(c, kept_end, n))) return rc;
    if ((rc = S->d_out.download(c, out_bytes, B))) return rc;
    CK_HIP(c, hipStreamSynchronize(st));
    if (n_kept) *n_kept = m;
    return CIRCKIT_OK;
}

}  // extern "C"
