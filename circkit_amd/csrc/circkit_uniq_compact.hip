// circkit_uniq_compact.hip -- the writer side of `circkit uniq` on the device (the reference's src/uniq.rs:47-66): the records
// that are the first with their hash, packed back to back into a new CSR batch, and the (duplicate, first occurrence) index
// pairs of the others.  Part of the uniq unit of include/circkit.h; the table and its kernels stay in circkit_uniq.hip, which
// this file reaches through the C ABI only.
//
// New device code here is one kernel: uniq_compact_decide_kernel turns first_seen and the record lengths into the word
// w[i] = WRITTEN | length (ck_compact::decide_uniq, monomer_compact.h).  Tile sums, scan of sums, apply (which also lists the
// dropped records), gather and the refusal of an overlapping output are the monomer compact's kernels, enqueued by
// ck_compact_launch (ck_compact_launch.h) with totals of this unit's own: circkit_monomers_status keeps answering for the last
// monomer compact, circkit_uniq_compact_status for the last uniq compact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "ck_compact_launch.h"
#include "monomer_compact.h"

namespace {

constexpr int DECIDE_WG = 256;                        // one lane per record
constexpr uint32_t DECIDE_MAX_GRID = 1u << 20;        // the lanes stride over the records beyond this many workgroups

__global__ __launch_bounds__(DECIDE_WG) void uniq_compact_decide_kernel(const uint64_t* __restrict__ offsets, uint64_t n,
                                                                        const uint64_t* __restrict__ first_seen, uint64_t base,
                                                                        uint64_t* __restrict__ w)
{
    const uint64_t stride = (uint64_t)gridDim.x * DECIDE_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * DECIDE_WG + threadIdx.x; i < n; i += stride)
        w[i] = ck_compact::decide_uniq(offsets[i + 1] - offsets[i], first_seen[i], base, i);
}

struct UniqCompactState {
    ck_totals totals;                    // [CK_COMPACT_WORDS], of the most recent uniq compact of this ctx
    // circkit_uniq_batch's staging
    ck_csr_buf in;
    ck_buf<uint8_t> d_canon, d_out;
    ck_buf<uint64_t> d_hash, d_fs, d_out_off, d_out_src;
};

UniqCompactState* state(circkit_ctx* c) { return ck_unit_state<UniqCompactState>(c, CK_UNIT_UNIQ_COMPACT); }

// the decide kernel and the shared kernels behind it, on the ctx stream; nothing waits
int launch(circkit_ctx* c, UniqCompactState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_first_seen,
           uint64_t base, uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src, uint64_t* d_dup_src, uint64_t* d_dup_first)
{
    uint64_t* d_w;
    const int rc = ck_compact_reserve(c, n, &d_w);
    if (rc) return rc;
    if (n) {
        uint64_t grid = (n + DECIDE_WG - 1) / DECIDE_WG;
        if (grid > DECIDE_MAX_GRID) grid = DECIDE_MAX_GRID;
        hipLaunchKernelGGL(uniq_compact_decide_kernel, dim3((uint32_t)grid), dim3(DECIDE_WG), 0, ck_ctx_stream(c), d_offsets, n, d_first_seen,
                           base, d_w);
    }
    return ck_compact_launch(c, &S->totals, d_bytes, d_offsets, n, d_out_bytes, d_out_offsets, d_out_src, d_dup_src, d_dup_first, d_first_seen);
}

int check_totals(circkit_ctx* c, const uint64_t* t)
{
    if (t[CK_COMPACT_OVERLAP]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_bytes overlaps the input payload: nothing was written");
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_uniq_compact_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_first_seen,
                                uint64_t base_index, uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src, uint64_t* d_dup_src,
                                uint64_t* d_dup_first)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n && (!d_bytes || !d_offsets || !d_first_seen || !d_out_bytes || !d_out_offsets || !d_out_src))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    return launch(c, state(c), d_bytes, d_offsets, n, d_first_seen, base_index, d_out_bytes, d_out_offsets, d_out_src, d_dup_src, d_dup_first);
}

int circkit_uniq_compact_status(circkit_ctx* c, uint64_t* n_kept, uint64_t* kept_bytes)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    UniqCompactState* S = state(c);
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[CK_COMPACT_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->totals.h ? S->totals.h : none;
    if (n_kept) *n_kept = t[CK_COMPACT_RECORDS];
    if (kept_bytes) *kept_bytes = t[CK_COMPACT_BYTES];
    return check_totals(c, t);
}

int circkit_uniq_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, int canonical_out, uint8_t* out_bytes,
                       uint64_t* out_offsets, uint64_t* out_src, uint64_t* first_seen, uint64_t* n_kept)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!offsets || !out_offsets) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n >= 0xFFFFFFFFull) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "circkit_uniq_batch: n_records must be < 2^32 - 1");
    if (n && (!out_src || (offsets[n] > offsets[0] && (!bytes || !out_bytes)))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    uint64_t at = 0;
    if (ck_csr_walk(offsets, n, CK_CSR_NO_LIMIT, &at)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    UniqCompactState* S = state(c);
    if (n_kept) *n_kept = 0;
    int rc;
    if (n == 0) {                        // an empty batch is a compact too: the status call reports its totals
        if ((rc = launch(c, S, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr))) return rc;
        CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
        out_offsets[0] = 0;
        return CIRCKIT_OK;
    }
    const uint64_t nb = offsets[n];
    if ((rc = S->in.upload(c, bytes, offsets, n))) return rc;
    if (canonical_out && (rc = S->d_canon.grow(c, nb))) return rc;
    if ((rc = S->d_hash.grow(c, n))) return rc;
    if ((rc = S->d_fs.grow(c, n))) return rc;
    if ((rc = S->d_out.grow(c, nb))) return rc;
    if ((rc = S->d_out_off.grow(c, n + 1))) return rc;
    if ((rc = S->d_out_src.grow(c, n))) return rc;
    uint8_t* const d_canon = canonical_out ? S->d_canon.p : nullptr;
    if ((rc = circkit_canonicalize_batch_device(c, S->in.bytes, S->in.off, n, d_canon, nullptr, nullptr, S->d_hash))) return rc;
    if ((rc = circkit_uniq_resolve_device(c, S->d_hash, n, 0, S->d_fs, nullptr))) return rc;
    if ((rc = launch(c, S, d_canon ? d_canon : S->in.bytes.p, S->in.off, n, S->d_fs, 0, S->d_out, S->d_out_off, S->d_out_src, nullptr, nullptr)))
        return rc;
    // three waits on a stream that has run dry after the first: a record the canonicalize left alone, keys that found no slot
    uint32_t unprocessed = 0;
    if ((rc = circkit_ctx_batch_status(c, &unprocessed))) return rc;
    if ((rc = circkit_uniq_status(c, nullptr))) return rc;
    if ((rc = check_totals(c, S->totals.h))) return rc;
    const uint64_t m = S->totals.h[CK_COMPACT_RECORDS], B = S->totals.h[CK_COMPACT_BYTES];
    if ((rc = S->d_out_off.download(c, out_offsets, m + 1))) return rc;
    if ((rc = S->d_out_src.download(c, out_src, m))) return rc;
    if ((rc = S->d_fs.download(c, first_seen, n))) return rc;
    if ((rc = S->d_out.download(c, out_bytes, B))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    if (n_kept) *n_kept = m;
    return CIRCKIT_OK;
}

}  // extern "C"
