// circkit_distance.hip -- the bounded edit distance of pairs of records of two CSR batches: the "edit distance of record pairs"
// section of include/circkit.h.  The routines are distance.h's; here are the kernel around them, the unit's state and the ABI.
//
// A pairs call is one launch on the ctx stream: distance_pairs_kernel, one wave per pair (striding over a fixed grid), each wave
// with SLICE_WORDS words of LDS.  Nothing waits and no workgroup waits for another.  The totals are the unit's own: they stay in
// device memory and are copied to page-locked memory behind the work, and circkit_distance_status answers from them whatever other
// unit ran in between.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "distance.h"

using ck_distance::Distance;
using ck_distance::DISTANCE_WAVES;
using ck_distance::SLICE_WORDS;
using ck_distance::T_WORDS;

static_assert(sizeof(circkit_distance_params) == 16, "params layout");
static_assert(CIRCKIT_DISTANCE_OVER == ck_distance::OVER && CIRCKIT_DISTANCE_MAX == ck_distance::DISTANCE_MAX, "the header's constants are the routines'");
static_assert(2 * ((2 * ck_distance::DISTANCE_MAX + 3 + 3) & ~3u) + ck_distance::STAGE_SLACK / 4 < SLICE_WORDS, "the rows of the widest cutoff fit the slice");

namespace {

constexpr uint32_t DISTANCE_MAX_GRID = 2048;           // workgroups of the pairs kernel: 8 a CU fill 256 CUs; the waves stride over the pairs

__global__ __launch_bounds__(64 * DISTANCE_WAVES) void distance_pairs_kernel(Distance D)
{
    __shared__ __attribute__((aligned(16))) uint32_t distance_lds[DISTANCE_WAVES * SLICE_WORDS];
    ck_distance::pairs_wave(D, distance_lds + ck::wave_in_block() * SLICE_WORDS, (uint64_t)blockIdx.x * DISTANCE_WAVES + ck::wave_in_block(),
                            (uint64_t)gridDim.x * DISTANCE_WAVES);
}

struct DistanceState {
    ck_totals totals;                // [T_WORDS], of the most recent pairs call
    bool any = false;
    // the staging of circkit_distance_pairs
    ck_csr_buf in[2];
    ck_buf<uint32_t> d_pairs, d_distance, d_scores;
};

int state(circkit_ctx* c, DistanceState** out)
{
    DistanceState* S = *out = ck_unit_state<DistanceState>(c, CK_UNIT_DISTANCE);
    return ck_totals_make(c, &S->totals, T_WORDS);
}

int check_params(circkit_ctx* c, const circkit_distance_params* p)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null distance params");
    if (p->max_distance > CIRCKIT_DISTANCE_MAX) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "max_distance must be 0 .. 255");
    if (p->reserved[0] || p->reserved[1] || p->reserved[2])
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved words of circkit_distance_params must be 0");
    return CIRCKIT_OK;
}

// the launch and the copy of the totals; the arguments are checked
int launch_pairs(circkit_ctx* c, DistanceState* S, const uint8_t* d_bytes_a, const uint64_t* d_offsets_a, uint64_t n_a, const uint8_t* d_bytes_b,
                 const uint64_t* d_offsets_b, uint64_t n_b, const circkit_distance_params& p, const uint32_t* d_pairs, uint64_t n_pairs,
                 uint32_t* d_out_distance, uint32_t* d_out_scores)
{
    hipStream_t st = ck_ctx_stream(c);
    int rc;
    if ((rc = ck_totals_clear(c, &S->totals, T_WORDS))) return rc;
    if (n_pairs) {
        Distance D;
        D.bytes_a = d_bytes_a; D.offsets_a = d_offsets_a; D.n_a = n_a;
        D.bytes_b = d_bytes_b; D.offsets_b = d_offsets_b; D.n_b = n_b;
        D.max_distance = p.max_distance;
        D.pairs = d_pairs; D.n_pairs = n_pairs;
        D.distance = d_out_distance; D.scores = d_out_scores; D.totals = S->totals.d;
        const uint64_t blocks = (n_pairs + DISTANCE_WAVES - 1) / DISTANCE_WAVES;
        hipLaunchKernelGGL(distance_pairs_kernel, dim3((uint32_t)(blocks > DISTANCE_MAX_GRID ? DISTANCE_MAX_GRID : blocks)), dim3(64 * DISTANCE_WAVES), 0, st, D);
        CK_HIP(c, hipGetLastError());
    }
    if ((rc = ck_totals_fetch(c, &S->totals, T_WORDS))) return rc;
    S->any = true;
    return CIRCKIT_OK;
}

int check_invalid(circkit_ctx* c, uint64_t n_invalid)
{
    if (n_invalid)
        return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu pairs name a record that does not exist or has 2^31 symbols or more and got no distance",
                       (unsigned long long)n_invalid);
    return CIRCKIT_OK;
}

// a host batch from its offsets alone, before a payload byte is read
int check_host_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n)
{
    if (n >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_a and n_b must be < 2^32");
    if (n && !offsets) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n && offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    uint64_t at = 0;
    const ck_csr_fault fault = ck_csr_walk(offsets, n, ck_sketch::TOO_LONG, &at);
    if (fault == CK_CSR_DECREASE) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (fault) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "record %llu has 2^31 symbols or more: no distance was computed", (unsigned long long)at);
    if (n && offsets[n] && !bytes) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_distance_pairs_device(circkit_ctx* c, const uint8_t* d_bytes_a, const uint64_t* d_offsets_a, uint64_t n_a, const uint8_t* d_bytes_b,
                                  const uint64_t* d_offsets_b, uint64_t n_b, const circkit_distance_params* params, const uint32_t* d_pairs,
                                  uint64_t n_pairs, uint32_t* d_out_distance, uint32_t* d_out_scores)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_a >= (1ull << 32) || n_b >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_a and n_b must be < 2^32");
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    if (n_pairs && (!d_pairs || (!d_out_distance && !d_out_scores))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_pairs && ((n_a && (!d_bytes_a || !d_offsets_a)) || (n_b && (!d_bytes_b || !d_offsets_b)))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_offsets_a & 7u) || ((uintptr_t)d_offsets_b & 7u) || ((uintptr_t)d_pairs & 3u) || ((uintptr_t)d_out_distance & 3u) ||
        ((uintptr_t)d_out_scores & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_offsets_a and d_offsets_b must be 8-byte aligned, d_pairs, d_out_distance and d_out_scores 4-byte aligned");
    const uint64_t off_a_bytes = (n_a + 1) * sizeof(uint64_t), off_b_bytes = (n_b + 1) * sizeof(uint64_t), pair_bytes = n_pairs * 2 * sizeof(uint32_t),
                   dist_bytes = n_pairs * sizeof(uint32_t);
    const void* outs[2] = { d_out_distance, d_out_scores };
    const uint64_t out_bytes[2] = { dist_bytes, pair_bytes };
    for (int o = 0; o < 2; ++o)
        if (ck_overlap(outs[o], out_bytes[o], d_offsets_a, off_a_bytes) || ck_overlap(outs[o], out_bytes[o], d_offsets_b, off_b_bytes) ||
            ck_overlap(outs[o], out_bytes[o], d_pairs, pair_bytes))
            return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_distance / d_out_scores overlap the offsets or the pairs");
    if (ck_overlap(d_out_distance, dist_bytes, d_out_scores, pair_bytes)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_distance overlaps d_out_scores");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    DistanceState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_pairs(c, S, d_bytes_a, d_offsets_a, n_a, d_bytes_b, d_offsets_b, n_b, *params, d_pairs, n_pairs, d_out_distance, d_out_scores);
}

int circkit_distance_status(circkit_ctx* c, uint64_t* n_within, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    DistanceState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0 };
    const uint64_t* t = S->any ? S->totals.h : none;
    if (n_within) *n_within = t[ck_distance::T_WITHIN];
    if (n_invalid) *n_invalid = t[ck_distance::T_INVALID];
    return check_invalid(c, t[ck_distance::T_INVALID]);
}

int circkit_distance_pairs(circkit_ctx* c, const uint8_t* bytes_a, const uint64_t* offsets_a, uint64_t n_a, const uint8_t* bytes_b,
                           const uint64_t* offsets_b, uint64_t n_b, const circkit_distance_params* params, const uint32_t* pairs, uint64_t n_pairs,
                           uint32_t* out_distance, uint32_t* out_scores)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    if (n_pairs && (!pairs || (!out_distance && !out_scores))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    const bool same = bytes_a == bytes_b && offsets_a == offsets_b && n_a == n_b;            // one batch: it is copied once
    if ((rc = check_host_batch(c, bytes_a, offsets_a, n_a))) return rc;
    if (!same && (rc = check_host_batch(c, bytes_b, offsets_b, n_b))) return rc;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    DistanceState* S;
    if ((rc = state(c, &S))) return rc;
    if ((rc = S->in[0].upload(c, bytes_a, offsets_a, n_a))) return rc;
    if (!same && (rc = S->in[1].upload(c, bytes_b, offsets_b, n_b))) return rc;
    if ((rc = S->d_pairs.upload(c, pairs, 2 * n_pairs))) return rc;
    if ((rc = S->d_distance.grow(c, n_pairs))) return rc;
    if ((rc = S->d_scores.grow(c, 2 * n_pairs))) return rc;
    const ck_csr_buf& b = S->in[same ? 0 : 1];
    if ((rc = launch_pairs(c, S, S->in[0].bytes, S->in[0].off, n_a, b.bytes, b.off, n_b, *params, S->d_pairs, n_pairs,
                           out_distance ? S->d_distance.p : nullptr, out_scores ? S->d_scores.p : nullptr)))
        return rc;
    if ((rc = S->d_distance.download(c, out_distance, n_pairs))) return rc;
    if ((rc = S->d_scores.download(c, out_scores, 2 * n_pairs))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    return check_invalid(c, S->totals.h[ck_distance::T_INVALID]);
}

}  // extern "C"
