// circkit_fasta_write.hip -- FASTA text written on the device: the "FASTA text from the device" section of include/circkit.h.
// The routines are fasta_write.h's; here are the kernels around them and the ABI.
//
// A write is five launches on the ctx stream, nothing waits and no workgroup waits for another:
//   fwrite_lengths_kernel    one lane per output record: out_offsets[k + 1] = the bytes record k writes (record_length: 0 for an
//                            invalid record), invalid records counted
//   fwrite_tile_sums_kernel  the sum of each tile of SCAN_TILE lengths
//   fwrite_scan_sums_kernel  one workgroup: the tile sums become exclusive, SCAN_WG of them a round; then the total, its
//                            comparison with the capacity and the refusal of an output that overlaps the text or the body
//   fwrite_apply_kernel      out_offsets in place: the lengths become the offsets
//   fwrite_write_kernel      write_tile over the output tiles, unless the scan refused the write
// The three scan kernels are ck_scan.h's bodies with fasta_write.h's SCAN_WG, SCAN_ITEMS and the saturating sum, so out_offsets
// never decreases.  The totals are this unit's own: they stay in device memory and are copied to page-locked memory
// behind the write, and circkit_fasta_write_status answers from them whatever parse, gather or translate ran in between.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "ck_scan.h"
#include "fasta_write.h"

using ck_fwrite::Label;
using ck_fwrite::Source;
using ck_fwrite::Span;

static_assert(sizeof(Span) == sizeof(circkit_fasta_span) && sizeof(Span) == 16, "device span layout");
static_assert(sizeof(Label) == sizeof(circkit_window) && sizeof(Label) == 24, "device window layout");

namespace {

constexpr int LEN_WG = 256;                            // lengths: one lane per record
constexpr int SCAN_WG = (int)ck_fwrite::SCAN_WG, SCAN_ITEMS = (int)ck_fwrite::SCAN_ITEMS, SCAN_TILE = (int)ck_fwrite::SCAN_TILE;
constexpr uint32_t LEN_MAX_GRID = 1u << 20;            // the lanes stride over the records beyond this many workgroups
constexpr uint32_t WRITE_GRID = 2048;                  // workgroups of the write: 8 per CU, striding over the output tiles
enum { T_TOTAL, T_INVALID, T_REFUSED, T_WORDS };       // the totals of a write, in device memory

// the body payload's ends are on the device
__device__ inline Source with_payload(Source S, uint64_t m)
{
    S.b0 = S.body && m ? S.body_offsets[0] : 0;
    S.b1 = S.body && m ? S.body_offsets[m] : 0;
    return S;
}

__global__ __launch_bounds__(LEN_WG) void fwrite_lengths_kernel(Source src, uint64_t m, uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ totals)
{
    const Source S = with_payload(src, m);
    const uint64_t stride = (uint64_t)gridDim.x * LEN_WG;
    for (uint64_t k = (uint64_t)blockIdx.x * LEN_WG + threadIdx.x; k < m; k += stride) {
        bool invalid;
        out_offsets[k + 1] = ck_fwrite::record_length(S, k, &invalid);
        if (invalid) atomicAdd((unsigned long long*)&totals[T_INVALID], 1ull);
    }
}

__global__ __launch_bounds__(SCAN_WG) void fwrite_tile_sums_kernel(const uint64_t* __restrict__ len, uint64_t m, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    const uint64_t total = ck_scan::tile_sum<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, len, m, [](uint64_t w) { return w; }, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the tile sums become exclusive, SCAN_WG of them a round; then the total, out_offsets[0] and the verdict.
__global__ __launch_bounds__(SCAN_WG) void fwrite_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles, Source src, uint64_t m, const uint8_t* out,
                                                                   uint64_t capacity, uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ totals)
{
    __shared__ uint64_t lds[SCAN_WG];
    const uint64_t total = ck_scan::sums_exclusive<SCAN_WG, ck_scan::SatAdd>(threadIdx.x, sums, n_tiles, lds);
    if (threadIdx.x == 0) {
        const Source S = with_payload(src, m);
        totals[T_TOTAL] = total;
        totals[T_REFUSED] = ck_fwrite::verdict(total, capacity, S.text, S.n_text, S.body, S.b0, S.b1, out);
        out_offsets[0] = 0;
    }
}

// out_offsets[k + 1]: record k's length becomes where it ends
__global__ __launch_bounds__(SCAN_WG) void fwrite_apply_kernel(uint64_t* __restrict__ ends, uint64_t m, const uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    ck_scan::apply_ends<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, ends, m, sums, lds);
}

__global__ __launch_bounds__(64 * ck_fwrite::WRITE_WAVES) void fwrite_write_kernel(Source src, uint64_t m, const uint64_t* __restrict__ out_offsets,
                                                                                   const uint64_t* __restrict__ totals, uint8_t* __restrict__ out)
{
    if (totals[T_REFUSED]) return;                    // the same for the whole grid
    ck_fwrite::Write W;
    W.S = with_payload(src, m);
    W.out_offsets = out_offsets;
    W.m = m; W.B = totals[T_TOTAL];
    W.out = out;
    if (W.B == 0) return;
    const uint64_t n_gran = (((uint64_t)(uintptr_t)out & 15u) + W.B + 15) / 16;
    const uint64_t n_tiles = (n_gran + ck_fwrite::TILE_GRANULES - 1) / ck_fwrite::TILE_GRANULES;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ck_fwrite::write_tile(W, t);
}

struct WriteState {
    ck_totals totals;                // [T_WORDS], made with the state
    uint64_t capacity = 0;           // of the most recent write, for the status message
    bool any = false;
    ck_buf<uint64_t> d_sums;
    // the staging of circkit_fasta_write_text
    ck_buf<uint8_t> d_text, d_out;
    ck_buf<Span> d_head, d_raw;
    ck_buf<uint64_t> d_src, d_out_off;
    ck_buf<Label> d_labels;
    ck_csr_buf body;
};

int state(circkit_ctx* c, WriteState** out)
{
    WriteState* S = *out = ck_unit_state<WriteState>(c, CK_UNIT_FASTA_WRITE);
    return ck_totals_make(c, &S->totals, T_WORDS);
}

// what both forms refuse before anything is enqueued
int check_args(circkit_ctx* c, const void* text, uint64_t n_text, const void* head, const void* raw, uint64_t n_heads, const void* src, uint64_t n_src,
               const void* body, const void* body_offsets, uint64_t n_out)
{
    if ((body != nullptr) != (body_offsets != nullptr)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_body and d_body_offsets go together");
    if ((body && raw) || (n_out && n_heads && !body && !raw))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "exactly one of d_body (with d_body_offsets) and d_raw must be given");
    if (n_out && n_heads && !head) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_text && !text) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (!src && n_src != n_heads) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "without d_src, n_src must be n_heads");
    if (n_text > (1ull << 40) || n_out >= (1ull << 40) || n_heads >= (1ull << 40) || n_src >= (1ull << 40))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_text, n_heads, n_src or n_out too large");
    return CIRCKIT_OK;
}

// lengths, the scan with its refusals; out_offsets is complete once the stream has run past it.  d_out is only compared.
int launch_offsets(circkit_ctx* c, WriteState* S, const Source& src, uint64_t m, const uint8_t* d_out, uint64_t capacity, uint64_t* d_out_offsets)
{
    const uint64_t tiles = (m + SCAN_TILE - 1) / SCAN_TILE;
    int rc;
    if ((rc = S->d_sums.grow(c, tiles))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, &S->totals, T_WORDS))) return rc;
    if (m) {
        const uint64_t grid = (m + LEN_WG - 1) / LEN_WG;
        hipLaunchKernelGGL(fwrite_lengths_kernel, dim3((uint32_t)(grid > LEN_MAX_GRID ? LEN_MAX_GRID : grid)), dim3(LEN_WG), 0, st, src, m, d_out_offsets,
                           S->totals.d);
        hipLaunchKernelGGL(fwrite_tile_sums_kernel, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, (const uint64_t*)d_out_offsets + 1, m, S->d_sums);
    }
    hipLaunchKernelGGL(fwrite_scan_sums_kernel, dim3(1), dim3(SCAN_WG), 0, st, S->d_sums, tiles, src, m, d_out, capacity, d_out_offsets, S->totals.d);
    if (m) hipLaunchKernelGGL(fwrite_apply_kernel, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, d_out_offsets + 1, m, (const uint64_t*)S->d_sums);
    CK_HIP(c, hipGetLastError());
    S->capacity = capacity;
    S->any = true;
    return CIRCKIT_OK;
}

int launch_write(circkit_ctx* c, WriteState* S, const Source& src, uint64_t m, const uint64_t* d_out_offsets, uint8_t* d_out)
{
    if (!m || !d_out) return CIRCKIT_OK;               // no record writes a byte
    hipLaunchKernelGGL(fwrite_write_kernel, dim3(WRITE_GRID), dim3(64 * ck_fwrite::WRITE_WAVES), 0, ck_ctx_stream(c), src, m, d_out_offsets,
                       (const uint64_t*)S->totals.d, d_out);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// the verdict on totals the stream has delivered
int check_totals(circkit_ctx* c, const uint64_t* t, uint64_t capacity)
{
    if (t[T_REFUSED] == ck_fwrite::REFUSED_CAPACITY)
        return ck_fail(c, CIRCKIT_ERR_OOM, "the records write %llu bytes of text, the buffer holds %llu: nothing was written", (unsigned long long)t[T_TOTAL],
                       (unsigned long long)capacity);
    if (t[T_REFUSED]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_text overlaps the text or the body payload: nothing was written");
    if (t[T_INVALID]) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu invalid records were written as zero bytes", (unsigned long long)t[T_INVALID]);
    return CIRCKIT_OK;
}

Source source_of(const uint8_t* text, uint64_t n_text, const circkit_fasta_span* head, const circkit_fasta_span* raw, uint64_t n_heads, const uint64_t* src,
                 uint64_t n_src, const circkit_window* labels, const uint8_t* body, const uint64_t* body_offsets)
{
    Source S;
    S.text = text; S.n_text = n_text;
    S.head = (const Span*)head; S.raw = (const Span*)raw; S.n_heads = n_heads;
    S.src = src; S.n_src = n_src;
    S.labels = (const Label*)labels;
    S.body = body; S.body_offsets = body_offsets;
    S.b0 = S.b1 = 0;                                   // the kernels read them
    return S;
}

}  // namespace

extern "C" {

int circkit_fasta_write_device(circkit_ctx* c, const uint8_t* d_text, uint64_t n_text, const circkit_fasta_span* d_head, const circkit_fasta_span* d_raw,
                               uint64_t n_heads, const uint64_t* d_src, uint64_t n_src, const circkit_window* d_labels, const uint8_t* d_body,
                               const uint64_t* d_body_offsets, uint64_t n_out, uint8_t* d_out_text, uint64_t out_capacity, uint64_t* d_out_offsets)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_args(c, d_text, n_text, d_head, d_raw, n_heads, d_src, n_src, d_body, d_body_offsets, n_out))) return rc;
    if (!d_out_offsets || (out_capacity && !d_out_text)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    WriteState* S;
    if ((rc = state(c, &S))) return rc;
    const Source src = source_of(d_text, n_text, d_head, d_raw, n_heads, d_src, n_src, d_labels, d_body, d_body_offsets);
    if ((rc = launch_offsets(c, S, src, n_out, d_out_text, out_capacity, d_out_offsets))) return rc;
    if ((rc = launch_write(c, S, src, n_out, d_out_offsets, d_out_text))) return rc;
    return ck_totals_fetch(c, &S->totals, T_WORDS);
}

int circkit_fasta_write_status(circkit_ctx* c, uint64_t* total_bytes, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    WriteState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->any ? S->totals.h : none;
    if (total_bytes) *total_bytes = t[T_TOTAL];
    if (n_invalid) *n_invalid = t[T_INVALID];
    return check_totals(c, t, S->capacity);
}

int circkit_fasta_write_text(circkit_ctx* c, const uint8_t* text, uint64_t n_text, const circkit_fasta_span* head, const circkit_fasta_span* raw,
                             uint64_t n_heads, const uint64_t* src, uint64_t n_src, const circkit_window* labels, const uint8_t* body,
                             const uint64_t* body_offsets, uint64_t n_out, uint8_t* out_text, uint64_t out_capacity, uint64_t* out_offsets, uint64_t* total)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_args(c, text, n_text, head, raw, n_heads, src, n_src, body, body_offsets, n_out))) return rc;
    if (!out_offsets) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    // the body as far as its offsets reach: they must not decrease, so that the last one is the payload's end
    uint64_t nb = 0;
    if (body_offsets) {
        uint64_t at = 0;
        if (ck_csr_walk(body_offsets, n_out, CK_CSR_NO_LIMIT, &at)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "body_offsets must not decrease");
        nb = body_offsets[n_out];
        if (nb >= (1ull << 48)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "body_offsets too large");
    }
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    WriteState* S;
    if ((rc = state(c, &S))) return rc;
    if ((rc = S->d_text.upload(c, text, n_text))) return rc;
    if ((rc = S->d_head.upload(c, (const Span*)head, n_heads))) return rc;
    if (raw && (rc = S->d_raw.upload(c, (const Span*)raw, n_heads))) return rc;
    if (src && (rc = S->d_src.upload(c, src, n_src))) return rc;
    if (labels && (rc = S->d_labels.upload(c, (const Label*)labels, n_out))) return rc;
    if (body && (rc = S->body.bytes.upload(c, body, nb))) return rc;
    if (body && (rc = S->body.off.upload(c, body_offsets, n_out + 1))) return rc;      // (all n_out + 1 of them, of no record too)
    if ((rc = S->d_out_off.grow(c, n_out + 1))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    const Source dev = source_of(S->d_text, n_text, (const circkit_fasta_span*)S->d_head.p, raw ? (const circkit_fasta_span*)S->d_raw.p : nullptr, n_heads,
                                 src ? S->d_src.p : nullptr, n_src, labels ? (const circkit_window*)S->d_labels.p : nullptr,
                                 body ? S->body.bytes.p : nullptr, body ? S->body.off.p : nullptr);
    // the offsets first: the staging for the text is sized by the total they end in (it cannot overlap the staged inputs)
    if ((rc = launch_offsets(c, S, dev, n_out, nullptr, out_capacity, S->d_out_off))) return rc;
    if ((rc = ck_totals_fetch(c, &S->totals, T_WORDS))) return rc;
    if ((rc = S->d_out_off.download(c, out_offsets, n_out + 1))) return rc;
    CK_HIP(c, hipStreamSynchronize(st));
    const uint64_t B = S->totals.h[T_TOTAL];
    if (total) *total = B;
    if (S->totals.h[T_REFUSED]) return check_totals(c, S->totals.h, out_capacity);
    if (B) {
        if (!out_text) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
        if ((rc = S->d_out.grow(c, B))) return rc;
        if ((rc = launch_write(c, S, dev, n_out, S->d_out_off, S->d_out))) return rc;
        if ((rc = S->d_out.download(c, out_text, B))) return rc;
        CK_HIP(c, hipStreamSynchronize(st));
    }
    return check_totals(c, S->totals.h, out_capacity);
}

}  // extern "C"
