// circkit_monomerize.hip -- `circkit monomerize` on the GPU: the entry points of include/circkit.h's monomerize section.
//
// monomerize_kernel: one wave per record runs ck_mono::record_end (monomerize.h) and lane 0 stores the record's end index
// (or CIRCKIT_MONOMER_NONE).  Nothing else is written: the monomer is a prefix of the input.  The record is read from
// global memory whatever its length (16-byte loads, contiguous across the wave); a 1 kb record is one scan step, a long one
// is walked by the same wave step by step.  Records of 2^32 symbols or more are not processed (NONE); the host form refuses
// the batch with CIRCKIT_ERR_TOO_LONG.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/circkit.h"
#include "ck_ctx.h"            // the ctx lives in circkit_hip.hip; this file sees it through this header
#include "monomerize.h"


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

struct MonoState {                   // host-buffer form staging (grow only)
    uint8_t* d_in = nullptr; uint64_t cap_in = 0;
    uint64_t* d_off = nullptr; uint64_t cap_off = 0;
    uint32_t* d_end = nullptr; uint64_t cap_end = 0;
};

void release_state(void* p)
{
    MonoState* S = (MonoState*)p;
    if (!S) return;
    void* ptrs[] = { S->d_in, S->d_off, S->d_end };
    for (void* q : ptrs) if (q) (void)hipFree(q);
    delete S;
}

MonoState* state(circkit_ctx* c)
{
    void** slot = ck_ctx_slot(c, CK_UNIT_MONOMERIZE, release_state);
    if (!*slot) *slot = new MonoState();
    return (MonoState*)*slot;
}

template <typename T>
int grow(circkit_ctx* c, T** p, uint64_t* cap, uint64_t want)
{
    if (want <= *cap) return CIRCKIT_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    CK_HIP(c, hipMalloc((void**)p, want * sizeof(T)));
    *cap = want;
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

}  // namespace

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
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
        if (offsets[i + 1] - offsets[i] > 0xFFFFFFFFull) return ck_ctx_fail(c, CIRCKIT_ERR_TOO_LONG, "a record of 2^32 symbols or more");
    }
    if (n == 0) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    MonoState* S = state(c);
    const uint64_t nb = offsets[n];
    if ((rc = grow(c, &S->d_in, &S->cap_in, nb ? nb : 1))) return rc;
    if ((rc = grow(c, &S->d_off, &S->cap_off, n + 1))) return rc;
    if ((rc = grow(c, &S->d_end, &S->cap_end, n))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if (nb) CK_HIP(c, hipMemcpyAsync(S->d_in, bytes, nb, hipMemcpyHostToDevice, st));
    CK_HIP(c, hipMemcpyAsync(S->d_off, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if ((rc = launch(c, S->d_in, S->d_off, n, P, S->d_end))) return rc;
    CK_HIP(c, hipMemcpyAsync(end, S->d_end, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    CK_HIP(c, hipStreamSynchronize(st));
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

}  // extern "C"
