// circkit_prealign.hip -- the rotation and strand of one circular record against another from their sketches and anchors: the
// "pre-alignment of circular records" section of include/circkit.h.  The routines are prealign.h's; here are the kernels around
// them, the unit's state and the ABI.
//
// A pairs call is one launch on the ctx stream: prealign_pairs_kernel, one wave per pair (striding), each wave with 1 << log2_bins
// words of LDS sized at the launch.  The pairs of labels are one more: prealign_labels_kernel, one lane per record (striding).
// Nothing waits and no workgroup waits for another.  The totals are the unit's own: they stay in device memory and are copied to
// page-locked memory behind the work, and circkit_prealign_status answers from them whatever other unit ran in between.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "prealign.h"

using ck_prealign::Prealign;
using ck_prealign::PREALIGN_WAVES;
using ck_prealign::T_WORDS;

static_assert(sizeof(circkit_prealign_params) == 16, "params layout");
static_assert(sizeof(circkit_window) == ck_prealign::WINDOW_BYTES, "window layout");
static_assert(CIRCKIT_ANCHOR_NONE == ck_prealign::NONE && CIRCKIT_ANCHOR_NONE == ck_sketch::ANCHOR_NONE, "the header's NONE is the routines'");

namespace {

constexpr uint32_t PAIRS_MAX_GRID = 8192;              // workgroups of the pairs kernel: the waves stride over the pairs
constexpr int LABELS_WG = 256;
constexpr uint32_t LABELS_MAX_GRID = 2048;             // of the labels kernel: the lanes stride over the records

__global__ __launch_bounds__(64 * PREALIGN_WAVES) void prealign_pairs_kernel(Prealign P)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t prealign_lds[];
    ck_prealign::pairs_wave(P, prealign_lds + ((size_t)ck::wave_in_block() << P.log2_bins), (uint64_t)blockIdx.x * PREALIGN_WAVES + ck::wave_in_block(),
                            (uint64_t)gridDim.x * PREALIGN_WAVES);
}

__global__ __launch_bounds__(LABELS_WG) void prealign_labels_kernel(const uint64_t* __restrict__ labels, uint64_t n, uint32_t* __restrict__ pairs)
{
    ck_prealign::labels_lane(labels, n, pairs, (uint64_t)blockIdx.x * LABELS_WG + threadIdx.x, (uint64_t)gridDim.x * LABELS_WG);
}

struct PrealignState {
    ck_totals totals;                // [T_WORDS], of the most recent pairs call
    bool any = false;
    // the staging of circkit_prealign_batch
    ck_csr_buf in;
    ck_buf<uint64_t> d_rows;
    ck_buf<uint32_t> d_anchors, d_pairs, d_scores;
    ck_buf<circkit_window> d_windows;
};

int state(circkit_ctx* c, PrealignState** out)
{
    PrealignState* S = *out = ck_unit_state<PrealignState>(c, CK_UNIT_PREALIGN);
    return ck_totals_make(c, &S->totals, T_WORDS);
}

int check_params(circkit_ctx* c, const circkit_prealign_params* p)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null prealign params");
    if (p->k < ck_sketch::K_MIN || p->k > ck_sketch::K_MAX) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "k must be 4 .. 32");
    if (p->log2_bins < ck_sketch::LOG2_BINS_MIN || p->log2_bins > ck_sketch::LOG2_BINS_MAX)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "log2_bins must be 4 .. 10");
    if (p->min_votes < 1) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "min_votes must be at least 1");
    if (p->reserved) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved word of circkit_prealign_params must be 0");
    return CIRCKIT_OK;
}

// the launch and the copy of the totals; the arguments are checked
int launch_pairs(circkit_ctx* c, PrealignState* S, const uint64_t* d_sketch, const uint32_t* d_anchors, const uint64_t* d_offsets, uint64_t n,
                 const circkit_prealign_params& p, const uint32_t* d_pairs, uint64_t n_pairs, circkit_window* d_windows, uint32_t* d_scores)
{
    hipStream_t st = ck_ctx_stream(c);
    int rc;
    if ((rc = ck_totals_clear(c, &S->totals, T_WORDS))) return rc;
    if (n_pairs) {
        Prealign P;
        P.rows = d_sketch; P.anchors = d_anchors; P.offsets = d_offsets; P.n_records = n;
        P.k = p.k; P.log2_bins = p.log2_bins; P.min_votes = p.min_votes;
        P.pairs = d_pairs; P.n_pairs = n_pairs;
        P.windows = (uint8_t*)d_windows; P.scores = d_scores; P.totals = S->totals.d;
        const size_t lds = ((size_t)PREALIGN_WAVES << p.log2_bins) * sizeof(uint32_t);
        hipLaunchKernelGGL(prealign_pairs_kernel, dim3(ck_grid_of(n_pairs, PREALIGN_WAVES, PAIRS_MAX_GRID)), dim3(64 * PREALIGN_WAVES), lds, st, P);
        CK_HIP(c, hipGetLastError());
    }
    if ((rc = ck_totals_fetch(c, &S->totals, T_WORDS))) return rc;
    S->any = true;
    return CIRCKIT_OK;
}

int check_invalid(circkit_ctx* c, uint64_t n_invalid)
{
    if (n_invalid)
        return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu pairs name a record that does not exist and got an empty window", (unsigned long long)n_invalid);
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_prealign_pairs_device(circkit_ctx* c, const uint64_t* d_sketch, const uint32_t* d_anchors, const uint64_t* d_offsets, uint64_t n_records,
                                  const circkit_prealign_params* params, const uint32_t* d_pairs, uint64_t n_pairs, circkit_window* d_windows,
                                  uint32_t* d_scores)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_records >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records must be < 2^32");
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    if (n_pairs && (!d_pairs || !d_windows || !d_scores)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_pairs && n_records && (!d_sketch || !d_anchors || !d_offsets)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_sketch & 7u) || ((uintptr_t)d_offsets & 7u) || ((uintptr_t)d_windows & 7u) || ((uintptr_t)d_anchors & 3u) ||
        ((uintptr_t)d_pairs & 3u) || ((uintptr_t)d_scores & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_sketch, d_offsets and d_windows must be 8-byte aligned, d_anchors, d_pairs and d_scores 4-byte aligned");
    const uint64_t row_bytes = (n_records << params->log2_bins) * sizeof(uint64_t), anchor_bytes = row_bytes / 2,
                   off_bytes = (n_records + 1) * sizeof(uint64_t), pair_bytes = n_pairs * 2 * sizeof(uint32_t),
                   window_bytes = n_pairs * sizeof(circkit_window);
    const void* outs[2] = { d_windows, d_scores };
    const uint64_t out_bytes[2] = { window_bytes, pair_bytes };
    for (int o = 0; o < 2; ++o)
        if (ck_overlap(outs[o], out_bytes[o], d_sketch, row_bytes) || ck_overlap(outs[o], out_bytes[o], d_anchors, anchor_bytes) ||
            ck_overlap(outs[o], out_bytes[o], d_offsets, off_bytes) || ck_overlap(outs[o], out_bytes[o], d_pairs, pair_bytes))
            return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_windows / d_scores overlap an input");
    if (ck_overlap(d_windows, window_bytes, d_scores, pair_bytes)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_windows overlaps d_scores");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    PrealignState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_pairs(c, S, d_sketch, d_anchors, d_offsets, n_records, *params, d_pairs, n_pairs, d_windows, d_scores);
}

int circkit_prealign_status(circkit_ctx* c, uint64_t* n_aligned, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    PrealignState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0 };
    const uint64_t* t = S->any ? S->totals.h : none;
    if (n_aligned) *n_aligned = t[ck_prealign::T_ALIGNED];
    if (n_invalid) *n_invalid = t[ck_prealign::T_INVALID];
    return check_invalid(c, t[ck_prealign::T_INVALID]);
}

int circkit_prealign_pairs_of_labels_device(circkit_ctx* c, const uint64_t* d_labels, uint64_t n_records, uint32_t* d_pairs)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n_records >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records must be < 2^32");
    if (n_records && (!d_labels || !d_pairs)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_labels & 7u) || ((uintptr_t)d_pairs & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_labels must be 8-byte aligned, d_pairs 4-byte aligned");
    if (ck_overlap(d_pairs, n_records * 2 * sizeof(uint32_t), d_labels, n_records * sizeof(uint64_t)))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_pairs overlaps d_labels");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    if (n_records) {
        hipLaunchKernelGGL(prealign_labels_kernel, dim3(ck_grid_of(n_records, LABELS_WG, LABELS_MAX_GRID)), dim3(LABELS_WG), 0, ck_ctx_stream(c), d_labels,
                           n_records, d_pairs);
        CK_HIP(c, hipGetLastError());
    }
    return CIRCKIT_OK;
}

int circkit_prealign_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, const circkit_sketch_params* sketch,
                           const uint32_t* pairs, uint64_t n_pairs, uint32_t min_votes, circkit_window* windows, uint32_t* scores)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!sketch) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null sketch params");
    if (sketch->reserved[0] || sketch->reserved[1]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved words of circkit_sketch_params must be 0");
    circkit_prealign_params p;
    p.k = sketch->k; p.log2_bins = sketch->log2_bins; p.min_votes = min_votes; p.reserved = 0;
    int rc;
    if ((rc = check_params(c, &p))) return rc;
    if (n_records >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records must be < 2^32");
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    if ((n_records && !offsets) || (n_pairs && (!pairs || !windows || !scores))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records && offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    // from the offsets alone, before a payload byte is read
    uint64_t at = 0;
    const ck_csr_fault fault = ck_csr_walk(offsets, n_records, ck_sketch::TOO_LONG, &at);
    if (fault == CK_CSR_DECREASE) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (fault) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "record %llu has 2^31 symbols or more: nothing was aligned", (unsigned long long)at);
    const uint64_t nb = n_records ? offsets[n_records] : 0;
    if (nb && !bytes) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    PrealignState* S;
    if ((rc = state(c, &S))) return rc;
    const uint64_t n_rows = n_records << sketch->log2_bins;
    if ((rc = S->in.upload(c, bytes, offsets, n_records))) return rc;
    if ((rc = S->d_rows.grow(c, n_rows))) return rc;
    if ((rc = S->d_anchors.grow(c, n_rows))) return rc;
    if ((rc = S->d_pairs.upload(c, pairs, 2 * n_pairs))) return rc;
    if ((rc = S->d_scores.grow(c, 2 * n_pairs))) return rc;
    if ((rc = S->d_windows.grow(c, n_pairs))) return rc;
    if ((rc = circkit_sketch_anchors_device(c, S->in.bytes, S->in.off, n_records, sketch, S->d_rows, nullptr, S->d_anchors))) return rc;
    if ((rc = launch_pairs(c, S, S->d_rows, S->d_anchors, S->in.off, n_records, p, S->d_pairs, n_pairs, S->d_windows, S->d_scores))) return rc;
    if ((rc = S->d_windows.download(c, windows, n_pairs))) return rc;
    if ((rc = S->d_scores.download(c, scores, 2 * n_pairs))) return rc;
    if ((rc = circkit_sketch_status(c, nullptr, nullptr))) return rc;   // (waits for the stream)
    return check_invalid(c, S->totals.h[ck_prealign::T_INVALID]);
}

}  // extern "C"
