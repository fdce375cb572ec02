// ck_ctx.h -- what a translation unit may ask of the ctx (internal; not part of the C ABI).
//
// struct circkit_ctx is defined in ck_ctx_impl.h, which only circkit_hip.hip (the ctx's lifecycle) and circkit_canon.hip (the
// canonicalize state, allocated with the ctx) include; nothing else names one of its fields.  The other units (one
// circkit_*.hip per ck_unit below, and circkit_bench.hip) enqueue on the ctx's stream, report through its error string and keep their own state behind
// one slot each, which circkit_ctx_destroy releases.  What that state is made of is here once: a grow-only device buffer that
// frees itself and stages host arrays (ck_buf, ck_csr_buf), the totals of a unit's most recent call (ck_totals), the typed
// slot (ck_unit_state), and the two small helpers the units share (ck_overlap, ck_grid_of).  The walk over a host batch's offsets is ck_csr.h.
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

// A device buffer that only grows, and its capacity: what a unit's state (and the ctx's own) is made of.  It frees itself, so a
// state struct lists its buffers once, as members.  Reads as the pointer it holds.
template <typename T>
struct ck_buf {
    T* p = nullptr;
    uint64_t cap = 0;                // elements
    ck_buf() = default;
    ck_buf(const ck_buf&) = delete;
    ck_buf& operator=(const ck_buf&) = delete;
    ~ck_buf() { release(); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // frees what it holds and owns q[n] instead
    void adopt(T* q, uint64_t n) { release(); p = q; cap = n; }
    // at least `want` elements afterwards, and never none (its contents are not kept)
    int grow(circkit_ctx* c, uint64_t want)
    {
        if (!want) want = 1;
        if (want <= cap) return CIRCKIT_OK;
        release();
        CK_HIP(c, hipMalloc((void**)&p, want * sizeof(T)));
        cap = want;
        return CIRCKIT_OK;
    }
    // grown for n elements, then src[n] copied in on the ctx stream (nothing is copied from a null src)
    int upload(circkit_ctx* c, const T* src, uint64_t n)
    {
        const int rc = grow(c, n);
        if (rc) return rc;
        if (n && src) CK_HIP(c, hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, ck_ctx_stream(c)));
        return CIRCKIT_OK;
    }
    // its first n elements copied to dst on the ctx stream (nothing to a null dst)
    int download(circkit_ctx* c, T* dst, uint64_t n) const
    {
        if (n && dst) CK_HIP(c, hipMemcpyAsync(dst, p, n * sizeof(T), hipMemcpyDeviceToHost, ck_ctx_stream(c)));
        return CIRCKIT_OK;
    }
};

// The staging of a host CSR batch: the payload and the n + 1 offsets, which the caller has checked (ck_csr.h).
struct ck_csr_buf {
    ck_buf<uint8_t> bytes;
    ck_buf<uint64_t> off;
    int upload(circkit_ctx* c, const uint8_t* src_bytes, const uint64_t* src_offsets, uint64_t n_records)
    {
        const int rc = bytes.upload(c, src_bytes, n_records ? src_offsets[n_records] : 0);
        if (rc) return rc;
        return n_records ? off.upload(c, src_offsets, n_records + 1) : off.grow(c, 1);
    }
};

// A unit's state in its slot: made on first use, deleted by circkit_ctx_destroy -- S's destructor is the only place that frees.
template <class S>
S* ck_unit_state(circkit_ctx* c, ck_unit unit)
{
    void** slot = ck_ctx_slot(c, unit, [](void* p) { delete static_cast<S*>(p); });
    if (!*slot) *slot = new S();
    return static_cast<S*>(*slot);
}

// [a, a + na) and [b, b + nb) share a byte (neither null nor empty)
inline bool ck_overlap(const void* a, uint64_t na, const void* b, uint64_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && na && nb && x < y + nb && y < x + na;
}

// the workgroups that take `work` items `per_block` at a time, at most max_grid of them (the kernel strides beyond)
inline uint32_t ck_grid_of(uint64_t work, uint32_t per_block, uint32_t max_grid)
{
    const uint64_t blocks = (work + per_block - 1) / per_block;
    return (uint32_t)(blocks > max_grid ? max_grid : blocks);
}

// Page-locked host memory that frees itself, and its capacity: staging the link copies from and into without a bounce, or
// (flags = hipHostMallocMapped) words a kernel writes and the host reads without waiting.
template <typename T>
struct ck_pinned {
    T* p = nullptr;
    uint64_t cap = 0;                // elements
    ck_pinned() = default;
    ck_pinned(const ck_pinned&) = delete;
    ck_pinned& operator=(const ck_pinned&) = delete;
    ~ck_pinned() { release(); }
    operator T*() const { return p; }
    void release() { if (p) (void)hipHostFree((void*)p); p = nullptr; cap = 0; }
    // at least `want` elements afterwards (its contents are not kept)
    int grow(circkit_ctx* c, uint64_t want, unsigned flags = hipHostMallocDefault)
    {
        if (want <= cap) return CIRCKIT_OK;
        release();
        CK_HIP(c, hipHostMalloc((void**)&p, want * sizeof(T), flags));
        cap = want;
        return CIRCKIT_OK;
    }
};

// The totals of a unit's most recent call: a few 64-bit words that the kernels write in device memory, and the same words in
// page-locked host memory, valid once the ctx stream has run past the copy.  How many words, and what they mean, is the unit's.
struct ck_totals {
    uint64_t* d = nullptr;
    uint64_t* h = nullptr;
    ck_totals() = default;
    ck_totals(const ck_totals&) = delete;
    ck_totals& operator=(const ck_totals&) = delete;
    ~ck_totals()
    {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
    }
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
