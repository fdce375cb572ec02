// circkit_sketch.hip -- MinHash sketches of circular records and their comparison: the "sketches of circular records" section of
// include/circkit.h.  The routines are sketch.h's; here are the kernels around them, the unit's state and the ABI.
//
// A sketch is two launches on the ctx stream, nothing waits and no workgroup waits for another:
//   sketch_short_kernel   one wave per record (striding): the row and count of a record of up to SKETCH_SEG symbols; a longer one gets
//                         an EMPTY row and count 0 and is appended to the ctx's list, or counted as unprocessed from 2^31 symbols on
//   sketch_long_kernel    a fixed grid over that list: the spans of every long record, merged into its row by the global minimum
// With anchors (circkit_sketch_anchors_device, the "pre-alignment" section) the first is anchors_short_kernel, which writes the anchor
// rows too, and a third follows: anchors_long_kernel, the same grid over the same list once the long rows are final.
// A compare is one launch: sketch_compare_kernel, one wave per pair (striding).
// The LDS of the first two is sized at the launch: SKETCH_WAVES slices of sketch.h's lds_words(log2_bins) 64-bit words.
// The totals of either kind are the unit's own: they stay in device memory and are copied to page-locked memory behind the work,
// and circkit_sketch_status / circkit_sketch_compare_status answer from them whatever other unit ran in between.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "sketch.h"

using ck_sketch::Anchors;
using ck_sketch::Compare;
using ck_sketch::Sketch;
using ck_sketch::SKETCH_WAVES;
using ck_sketch::T_WORDS;

static_assert(sizeof(circkit_sketch_params) == 24, "params layout");
static_assert(CIRCKIT_SKETCH_EMPTY == ck_sketch::EMPTY, "the header's EMPTY is the routines'");

namespace {

constexpr uint32_t SHORT_MAX_GRID = 8192;              // workgroups of the short kernel: 8 per CU and SIMD's worth, striding over the records
constexpr uint32_t LONG_GRID = 2048;                   // workgroups of the long kernel
constexpr uint32_t COMPARE_WAVES = 4, COMPARE_MAX_GRID = 1u << 16;

__global__ __launch_bounds__(64 * SKETCH_WAVES) void sketch_short_kernel(Sketch S)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sketch_lds[];
    ck_sketch::short_block(S, sketch_lds, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64 * SKETCH_WAVES) void sketch_long_kernel(Sketch S)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sketch_lds[];
    ck_sketch::long_block(S, sketch_lds, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64 * SKETCH_WAVES) void anchors_short_kernel(Anchors A)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sketch_lds[];
    ck_sketch::anchors_short_block(A, sketch_lds, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64 * SKETCH_WAVES) void anchors_long_kernel(Anchors A)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t sketch_lds[];
    ck_sketch::anchors_long_block(A, sketch_lds, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64 * COMPARE_WAVES) void sketch_compare_kernel(Compare C)
{
    ck_sketch::compare_wave(C, (uint64_t)blockIdx.x * COMPARE_WAVES + ck::wave_in_block(), (uint64_t)gridDim.x * COMPARE_WAVES);
}

struct SketchState {
    ck_totals totals;                // [T_WORDS], of the most recent sketch; both made with the state
    ck_totals invalid;               // [1]: the invalid pairs of the most recent compare
    bool any = false, any_compare = false;
    ck_buf<uint64_t> d_long;         // the list of long records (n_records entries)
    // the staging of the host forms
    ck_csr_buf in;
    ck_buf<uint64_t> d_rows, d_rows_b;
    ck_buf<uint32_t> d_counts, d_pairs, d_result;
};

int state(circkit_ctx* c, SketchState** out)
{
    SketchState* S = *out = ck_unit_state<SketchState>(c, CK_UNIT_SKETCH);
    int rc;
    if ((rc = ck_totals_make(c, &S->totals, T_WORDS))) return rc;
    return ck_totals_make(c, &S->invalid, 1);
}

int check_params(circkit_ctx* c, const circkit_sketch_params* p)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null sketch params");
    if (p->k < ck_sketch::K_MIN || p->k > ck_sketch::K_MAX) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "k must be 4 .. 32");
    if (p->log2_bins < ck_sketch::LOG2_BINS_MIN || p->log2_bins > ck_sketch::LOG2_BINS_MAX)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "log2_bins must be 4 .. 10");
    if (p->reserved[0] || p->reserved[1]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved words of circkit_sketch_params must be 0");
    return CIRCKIT_OK;
}

// the two launches (three with anchors) and the copy of the totals; the arguments are checked
int launch_sketch(circkit_ctx* c, SketchState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const circkit_sketch_params& p,
                  uint64_t* d_out, uint32_t* d_counts, uint32_t* d_anchors = nullptr)
{
    int rc;
    if ((rc = S->d_long.grow(c, n))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, &S->totals, T_WORDS))) return rc;
    if (n) {
        Sketch K;
        K.bytes = d_bytes; K.offsets = d_offsets; K.n_records = n;
        K.k = p.k; K.log2_bins = p.log2_bins; K.seed = p.seed;
        K.out = d_out; K.out_count = d_counts;
        K.long_list = S->d_long; K.totals = S->totals.d;
        const uint64_t blocks = (n + SKETCH_WAVES - 1) / SKETCH_WAVES;
        const size_t lds = (size_t)SKETCH_WAVES * ck_sketch::lds_words(p.log2_bins) * sizeof(uint64_t);
        const dim3 short_grid((uint32_t)(blocks > SHORT_MAX_GRID ? SHORT_MAX_GRID : blocks));
        if (d_anchors) {
            Anchors A;
            A.S = K; A.out_anchor = d_anchors;
            const size_t alds = (size_t)SKETCH_WAVES * ck_sketch::anchors_lds_words(p.log2_bins) * sizeof(uint64_t);
            hipLaunchKernelGGL(anchors_short_kernel, short_grid, dim3(64 * SKETCH_WAVES), alds, st, A);
            hipLaunchKernelGGL(sketch_long_kernel, dim3(LONG_GRID), dim3(64 * SKETCH_WAVES), lds, st, K);
            hipLaunchKernelGGL(anchors_long_kernel, dim3(LONG_GRID), dim3(64 * SKETCH_WAVES), alds, st, A);
        } else {
            hipLaunchKernelGGL(sketch_short_kernel, short_grid, dim3(64 * SKETCH_WAVES), lds, st, K);
            hipLaunchKernelGGL(sketch_long_kernel, dim3(LONG_GRID), dim3(64 * SKETCH_WAVES), lds, st, K);
        }
        CK_HIP(c, hipGetLastError());
    }
    if ((rc = ck_totals_fetch(c, &S->totals, T_WORDS))) return rc;
    S->any = true;
    return CIRCKIT_OK;
}

int check_totals(circkit_ctx* c, const uint64_t* t)
{
    if (t[ck_sketch::T_UNPROCESSED])
        return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "%llu records of 2^31 symbols or more were not sketched: their rows are empty",
                       (unsigned long long)t[ck_sketch::T_UNPROCESSED]);
    return CIRCKIT_OK;
}

int launch_compare(circkit_ctx* c, SketchState* S, const uint64_t* d_a, uint64_t n_a, const uint64_t* d_b, uint64_t n_b, uint32_t log2_bins,
                   const uint32_t* d_pairs, uint64_t n_pairs, uint32_t* d_out)
{
    hipStream_t st = ck_ctx_stream(c);
    int rc;
    if ((rc = ck_totals_clear(c, &S->invalid, 1))) return rc;
    if (n_pairs) {
        Compare C;
        C.a = d_a; C.b = d_b; C.n_a = n_a; C.n_b = n_b;
        C.log2_bins = log2_bins;
        C.pairs = d_pairs; C.n_pairs = n_pairs;
        C.out = d_out; C.n_invalid = S->invalid.d;
        const uint64_t blocks = (n_pairs + COMPARE_WAVES - 1) / COMPARE_WAVES;
        hipLaunchKernelGGL(sketch_compare_kernel, dim3((uint32_t)(blocks > COMPARE_MAX_GRID ? COMPARE_MAX_GRID : blocks)), dim3(64 * COMPARE_WAVES), 0, st, C);
        CK_HIP(c, hipGetLastError());
    }
    if ((rc = ck_totals_fetch(c, &S->invalid, 1))) return rc;
    S->any_compare = true;
    return CIRCKIT_OK;
}

int check_invalid(circkit_ctx* c, uint64_t n_invalid)
{
    if (n_invalid) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu invalid pairs were written as (0, 0)", (unsigned long long)n_invalid);
    return CIRCKIT_OK;
}

int check_compare_args(circkit_ctx* c, const void* a, const void* b, uint32_t log2_bins, const void* pairs, uint64_t n_pairs, const void* out)
{
    if (log2_bins < ck_sketch::LOG2_BINS_MIN || log2_bins > ck_sketch::LOG2_BINS_MAX)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "log2_bins must be 4 .. 10");
    if (n_pairs && (!a || !b || !pairs || !out)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_sketch_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records, const circkit_sketch_params* params,
                                uint64_t* d_out_sketch, uint32_t* d_out_n_kmers)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_records && (!d_bytes || !d_offsets || !d_out_sketch)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_out_sketch & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_out_n_kmers & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_offsets and d_out_sketch must be 8-byte aligned, d_out_n_kmers 4-byte aligned");
    if (n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    // the arrays whose extent the host knows; the payload's ends are the device's, and keeping the outputs off it is the caller's contract
    const uint64_t row_bytes = (n_records << params->log2_bins) * sizeof(uint64_t);
    if (ck_overlap(d_out_sketch, row_bytes, d_offsets, (n_records + 1) * sizeof(uint64_t)) ||
        ck_overlap(d_out_n_kmers, n_records * sizeof(uint32_t), d_offsets, (n_records + 1) * sizeof(uint64_t)) ||
        ck_overlap(d_out_sketch, row_bytes, d_out_n_kmers, n_records * sizeof(uint32_t)))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_sketch / d_out_n_kmers overlap the offsets or each other");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    SketchState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_sketch(c, S, d_bytes, d_offsets, n_records, *params, d_out_sketch, d_out_n_kmers);
}

int circkit_sketch_anchors_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records, const circkit_sketch_params* params,
                                  uint64_t* d_out_sketch, uint32_t* d_out_n_kmers, uint32_t* d_out_anchors)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_records && (!d_bytes || !d_offsets || !d_out_sketch || !d_out_anchors)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_out_sketch & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_out_n_kmers & 3u) || ((uintptr_t)d_out_anchors & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_offsets and d_out_sketch must be 8-byte aligned, d_out_n_kmers and d_out_anchors 4-byte aligned");
    if (n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    const uint64_t row_bytes = (n_records << params->log2_bins) * sizeof(uint64_t), anchor_bytes = row_bytes / 2,
                   off_bytes = (n_records + 1) * sizeof(uint64_t), count_bytes = n_records * sizeof(uint32_t);
    if (ck_overlap(d_out_sketch, row_bytes, d_offsets, off_bytes) || ck_overlap(d_out_n_kmers, count_bytes, d_offsets, off_bytes) ||
        ck_overlap(d_out_sketch, row_bytes, d_out_n_kmers, count_bytes) || ck_overlap(d_out_anchors, anchor_bytes, d_offsets, off_bytes) ||
        ck_overlap(d_out_anchors, anchor_bytes, d_out_sketch, row_bytes) || ck_overlap(d_out_anchors, anchor_bytes, d_out_n_kmers, count_bytes))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_sketch / d_out_n_kmers / d_out_anchors overlap the offsets or each other");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    SketchState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_sketch(c, S, d_bytes, d_offsets, n_records, *params, d_out_sketch, d_out_n_kmers, d_out_anchors);
}

int circkit_sketch_status(circkit_ctx* c, uint64_t* n_valid_kmers_total, uint32_t* n_unprocessed)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    SketchState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->any ? S->totals.h : none;
    if (n_valid_kmers_total) *n_valid_kmers_total = t[ck_sketch::T_VALID];
    if (n_unprocessed) *n_unprocessed = t[ck_sketch::T_UNPROCESSED] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t[ck_sketch::T_UNPROCESSED];
    return check_totals(c, t);
}

int circkit_sketch_compare_device(circkit_ctx* c, const uint64_t* d_sketch_a, uint64_t n_a, const uint64_t* d_sketch_b, uint64_t n_b, uint32_t log2_bins,
                                  const uint32_t* d_pairs, uint64_t n_pairs, uint32_t* d_out)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_compare_args(c, d_sketch_a, d_sketch_b, log2_bins, d_pairs, n_pairs, d_out))) return rc;
    if (((uintptr_t)d_sketch_a & 7u) || ((uintptr_t)d_sketch_b & 7u) || ((uintptr_t)d_pairs & 3u) || ((uintptr_t)d_out & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the sketches must be 8-byte aligned, d_pairs and d_out 4-byte aligned");
    const uint64_t out_bytes = n_pairs * 2 * sizeof(uint32_t);
    if (ck_overlap(d_out, out_bytes, d_pairs, out_bytes) || ck_overlap(d_out, out_bytes, d_sketch_a, (n_a << log2_bins) * sizeof(uint64_t)) ||
        ck_overlap(d_out, out_bytes, d_sketch_b, (n_b << log2_bins) * sizeof(uint64_t)))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out overlaps the pairs or a sketch");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    SketchState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_compare(c, S, d_sketch_a, n_a, d_sketch_b, n_b, log2_bins, d_pairs, n_pairs, d_out);
}

int circkit_sketch_compare_status(circkit_ctx* c, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    SketchState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t bad = S->any_compare ? S->invalid.h[0] : 0;
    if (n_invalid) *n_invalid = bad;
    return check_invalid(c, bad);
}

int circkit_sketch_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, const circkit_sketch_params* params,
                         uint64_t* out_sketch, uint32_t* out_n_kmers)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_records && (!offsets || !out_sketch)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    if (n_records && offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    // from the offsets alone, before a payload byte is read
    uint64_t at = 0;
    const ck_csr_fault fault = ck_csr_walk(offsets, n_records, ck_sketch::TOO_LONG, &at);
    if (fault == CK_CSR_DECREASE) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (fault) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "record %llu has 2^31 symbols or more: nothing was sketched", (unsigned long long)at);
    const uint64_t nb = n_records ? offsets[n_records] : 0;
    if (nb && !bytes) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    SketchState* S;
    if ((rc = state(c, &S))) return rc;
    const uint64_t n_rows = n_records << params->log2_bins;
    if ((rc = S->in.upload(c, bytes, offsets, n_records))) return rc;
    if ((rc = S->d_rows.grow(c, n_rows))) return rc;
    if ((rc = S->d_counts.grow(c, n_records))) return rc;
    if ((rc = launch_sketch(c, S, S->in.bytes, S->in.off, n_records, *params, S->d_rows, S->d_counts))) return rc;
    if ((rc = S->d_rows.download(c, out_sketch, n_rows))) return rc;
    if ((rc = S->d_counts.download(c, out_n_kmers, n_records))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    return check_totals(c, S->totals.h);
}

int circkit_sketch_compare(circkit_ctx* c, const uint64_t* sketch_a, uint64_t n_a, const uint64_t* sketch_b, uint64_t n_b, uint32_t log2_bins,
                           const uint32_t* pairs, uint64_t n_pairs, uint32_t* out)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_compare_args(c, sketch_a, sketch_b, log2_bins, pairs, n_pairs, out))) return rc;
    if (n_a >= (1ull << 40) || n_b >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_a or n_b too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    SketchState* S;
    if ((rc = state(c, &S))) return rc;
    const bool same = sketch_a == sketch_b;
    const uint64_t wa = (same && n_b > n_a ? n_b : n_a) << log2_bins, wb = same ? 0 : n_b << log2_bins;
    // (without pairs no row is read: the sketches may be null then)
    if ((rc = S->d_rows.upload(c, n_pairs ? sketch_a : nullptr, wa))) return rc;
    if ((rc = S->d_rows_b.upload(c, n_pairs ? sketch_b : nullptr, wb))) return rc;
    if ((rc = S->d_pairs.upload(c, pairs, 2 * n_pairs))) return rc;
    if ((rc = S->d_result.grow(c, 2 * n_pairs))) return rc;
    if ((rc = launch_compare(c, S, S->d_rows, n_a, same ? S->d_rows : S->d_rows_b, n_b, log2_bins, S->d_pairs, n_pairs, S->d_result))) return rc;
    if ((rc = S->d_result.download(c, out, 2 * n_pairs))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    return check_invalid(c, S->invalid.h[0]);
}

}  // extern "C"
