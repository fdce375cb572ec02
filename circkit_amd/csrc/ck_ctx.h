// ck_ctx.h -- what a translation unit may ask of the ctx (internal; not part of the C ABI).
//
// struct circkit_ctx is defined in ck_ctx_impl.h, which only circkit_hip.hip (the ctx's lifecycle) and circkit_canon.hip (the
// canonicalize state, allocated with the ctx) include; nothing else names one of its fields.  The other units (one
// circkit_*.hip per ck_unit below, and circkit_bench.hip) enqueue on the ctx's stream, report through its error string and keep their own state behind
// one slot each, which circkit_ctx_destroy releases.  What that state is made of is here once: a grow-only device buffer
// (ck_grow) and the totals of a unit's most recent call (ck_totals).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/circkit.h"

hipStream_t ck_ctx_stream(circkit_ctx* c);
int ck_ctx_device(circkit_ctx* c);
// the ctx's complement table on the device: 256 bytes, bio 1.3.1 alphabets::dna (what the canonicalize kernels read)
const uint8_t* ck_ctx_complement(circkit_ctx* c);

// the ctx's last-error string = the formatted message (c may be null); returns `code`
int ck_fail(circkit_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int ck_ctx_fail(circkit_ctx* c, int code, const char* msg) { return ck_fail(c, code, "%s", msg); }

#define CK_HIP(c, call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ck_fail(c, e_ == hipErrorOutOfMemory ? CIRCKIT_ERR_OOM : CIRCKIT_ERR_HIP,        \
                           "%s failed: %s", #call, hipGetErrorString(e_));                          \
    } while (0)

// One slot of state per unit: *slot is null until the unit puts its state there; circkit_ctx_destroy hands whatever it
// finds to the `release` the unit named.
enum ck_unit { CK_UNIT_ORFS, CK_UNIT_MONOMERIZE, CK_UNIT_UNIQ, CK_UNIT_UNIQ_COMPACT, CK_UNIT_WINDOWS, CK_UNIT_FASTA, CK_UNIT_FASTA_WRITE, CK_UNIT_SKETCH, CK_UNIT_CLUSTER, CK_UNIT_PREALIGN, CK_UNIT_DISTANCE, CK_N_UNITS };
void** ck_ctx_slot(circkit_ctx* c, ck_unit unit, void (*release)(void*));

// The uniq unit's overflow word on the device (circkit_uniq.hip): the records whose key found no slot since the table was last
// cleared, 32 bits.  A unit that runs circkit_uniq_resolve_device for its own ends copies the word behind the resolve, on the ctx
// stream, so that its status answers for its own resolve whatever uses the table afterwards.  *out stays valid for the ctx's life.
int ck_uniq_overflow_word(circkit_ctx* c, const uint32_t** out);

// A device buffer of a unit's state that only grows: *p holds at least `want` elements afterwards (its contents are not kept).
template <typename T>
int ck_grow(circkit_ctx* c, T** p, uint64_t* cap, uint64_t want)
{
    if (want <= *cap) return CIRCKIT_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    CK_HIP(c, hipMalloc((void**)p, want * sizeof(T)));
    *cap = want;
    return CIRCKIT_OK;
}

// The totals of a unit's most recent call: a few 64-bit words that the kernels write in device memory, and the same words in
// page-locked host memory, valid once the ctx stream has run past the copy.  How many words, and what they mean, is the unit's.
struct ck_totals {
    uint64_t* d = nullptr;
    uint64_t* h = nullptr;
};
// both where missing; new host words are 0
inline int ck_totals_make(circkit_ctx* c, ck_totals* T, int words)
{
    if (!T->d) CK_HIP(c, hipMalloc((void**)&T->d, words * sizeof(uint64_t)));
    if (!T->h) {
        CK_HIP(c, hipHostMalloc((void**)&T->h, words * sizeof(uint64_t), hipHostMallocDefault));
        for (int k = 0; k < words; ++k) T->h[k] = 0;
    }
    return CIRCKIT_OK;
}
// on the ctx stream: the device words become 0 in front of the work / are copied to the host words behind it
inline int ck_totals_clear(circkit_ctx* c, ck_totals* T, int words)
{
    CK_HIP(c, hipMemsetAsync(T->d, 0, words * sizeof(uint64_t), ck_ctx_stream(c)));
    return CIRCKIT_OK;
}
inline int ck_totals_fetch(circkit_ctx* c, ck_totals* T, int words)
{
    CK_HIP(c, hipMemcpyAsync(T->h, T->d, words * sizeof(uint64_t), hipMemcpyDeviceToHost, ck_ctx_stream(c)));
    return CIRCKIT_OK;
}
inline void ck_totals_release(ck_totals* T)
{
    if (T->d) (void)hipFree(T->d);
    if (T->h) (void)hipHostFree(T->h);
    T->d = T->h = nullptr;
}
