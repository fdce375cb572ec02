// circkit_uniq.hip -- the `uniq` first-seen table: its kernels and the circkit_uniq_* entry points of include/circkit.h.
// Nothing here is shared with the canonicalize path.  The ctx lives in circkit_hip.hip; this file sees it through ck_ctx.h and
// keeps the table, its status words and the host form's staging in a UniqState of its own behind the ctx's uniq slot.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/circkit.h"
#include "ck_ctx.h"
#include "wave_prims.h"

namespace {

// uniq: open-addressing table keyed by the 64-bit hash, value = smallest global record index.  One 16-byte slot
// {key, value} per entry, so that claiming a key and folding its index touch ONE 64-byte sector (two arrays: two
// random DRAM accesses per key).  Slot [mask + 1] keeps the value of the key that equals the EMPTY marker.
constexpr uint64_t UNIQ_EMPTY = ~0ull;
struct __attribute__((aligned(16))) UniqSlot { unsigned long long key, val; };
__device__ __forceinline__ uint64_t uniq_slot(uint64_t h, uint64_t mask) { return (h ^ (h >> 29)) & mask; }
__device__ __forceinline__ UniqSlot uniq_peek(const UniqSlot* p)
{
    typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
    const v2 v = *reinterpret_cast<const v2*>(p);          // one global_load_dwordx4
    return UniqSlot{ v.x, v.y };
}
// Folds (h, v) into the table.  The scattered device-scope atomics are the limiter (~20 G/s chip-wide, measured:
// 10M keys x CAS + min = 1.08 ms), so a plain 16-byte read goes first: a key that is already there with a smaller
// value -- the later copies of a duplicated record, since threads take records roughly in index order -- needs no
// atomic at all, a present key one, a new key two.  The read may be stale; it is only trusted where staleness cannot
// hurt: a key, once written, never changes, and a value only decreases.
__device__ __forceinline__ bool uniq_fold(UniqSlot* t, uint64_t mask, uint64_t h, unsigned long long v)
{
    if (h == UNIQ_EMPTY) { atomicMin(&t[mask + 1].val, v); return true; }
    uint64_t s = uniq_slot(h, mask), probes = 0;
    for (;;) {
        const UniqSlot cur = uniq_peek(t + s);
        if (cur.key == h) {
            if (cur.val > v) atomicMin(&t[s].val, v);
            return true;
        }
        if (cur.key == UNIQ_EMPTY) {
            const unsigned long long old = atomicCAS(&t[s].key, (unsigned long long)UNIQ_EMPTY, (unsigned long long)h);
            if (old == UNIQ_EMPTY || old == h) { atomicMin(&t[s].val, v); return true; }
        }
        s = (s + 1) & mask;
        if (++probes > mask) return false;                  // table full
    }
}

// The value the table holds for key h; EMPTY when it holds none (the key was never folded in, or found no slot in a full table:
// the probe gives up after a full circle).  One exit: with an early return the compiler schedules the lookup kernels differently.
__device__ __forceinline__ uint64_t uniq_find(const UniqSlot* t, uint64_t mask, uint64_t h)
{
    uint64_t r = UNIQ_EMPTY;
    if (h == UNIQ_EMPTY) {
        r = t[mask + 1].val;
    } else {
        uint64_t s = uniq_slot(h, mask), probes = 0;
        for (;;) {
            const UniqSlot cur = uniq_peek(t + s);
            if (cur.key == h) { r = cur.val; break; }
            if (cur.key == UNIQ_EMPTY || ++probes > mask) break;
            s = (s + 1) & mask;
        }
    }
    return r;
}

// value of key i: index[i] when given (pairs gathered from other ranks), else base + i (a shard in input order)
__global__ __launch_bounds__(256) void uniq_insert_kernel(const uint64_t* __restrict__ hash, const uint64_t* __restrict__ index, uint64_t n, uint64_t base,
                                                          UniqSlot* t, uint64_t mask, uint32_t* status)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (!uniq_fold(t, mask, hash[i], index ? index[i] : base + i)) atomicAdd(status, 1u);
}

// keep (nullable): keep[i] = 1 iff record base + i is the first with its hash -- the reference's "emit or table row"
// decision (src/uniq.rs:47-62) for a shard whose record i has global index base + i
__global__ __launch_bounds__(256) void uniq_lookup_kernel(const uint64_t* __restrict__ hash, uint64_t n, const UniqSlot* __restrict__ t, uint64_t mask,
                                                          uint64_t* first_seen, uint8_t* keep, uint64_t base)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = uniq_find(t, mask, hash[i]);
        first_seen[i] = r;
        if (keep) keep[i] = r == base + i;
    }
}

// circkit_uniq_resolve_device's own pair of kernels: one shard, one insert pass, one lookup pass, LOCAL indices
// (i < 2^32 - 1: 0xFFFFFFFF is the "nothing yet" value of either half).  The value word is split: its high half receives the index of the record that CLAIMED the key -- a plain
// store, the claimer needs no second atomic --, its low half the smallest index among the records that found the key
// present (32-bit atomicMin, skipped when the peek already shows a smaller index in either half).  first-seen =
// min(low, high).  With threads taking records roughly in index order a key costs ONE atomic (the CAS) instead of two:
// 10M records, half of them duplicates: 507 -> ~350 us (the 207 us of peeks stay).
__device__ __forceinline__ bool uniq_fold_local(UniqSlot* t, uint64_t mask, uint64_t h, uint32_t i)
{
    if (h == UNIQ_EMPTY) { atomicMin(reinterpret_cast<unsigned int*>(&t[mask + 1].val), i); return true; }
    uint64_t s = uniq_slot(h, mask), probes = 0;
    for (;;) {
        const UniqSlot cur = uniq_peek(t + s);
        unsigned int* halves = reinterpret_cast<unsigned int*>(&t[s].val);      // [0] low, [1] high (little endian)
        if (cur.key == h) {
            const uint32_t lo = (uint32_t)cur.val, hi = (uint32_t)(cur.val >> 32);
            if ((lo < hi ? lo : hi) > i) atomicMin(halves, i);
            return true;
        }
        if (cur.key == UNIQ_EMPTY) {
            const unsigned long long old = atomicCAS(&t[s].key, (unsigned long long)UNIQ_EMPTY, (unsigned long long)h);
            if (old == UNIQ_EMPTY) { halves[1] = i; return true; }             // ours: nobody else writes this half
            if (old == h) { atomicMin(halves, i); return true; }
        }
        s = (s + 1) & mask;
        if (++probes > mask) return false;                  // table full
    }
}
__global__ __launch_bounds__(256) void uniq_resolve_insert_kernel(const uint64_t* __restrict__ hash, uint64_t n, UniqSlot* t, uint64_t mask, uint32_t* status,
                                                                  const uint32_t* only_if = nullptr)
{
    if (only_if && *only_if == 0) return;                   // (the bucketed resolve's fallback: runs only when a bucket was too big)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (!uniq_fold_local(t, mask, hash[i], (uint32_t)i)) atomicAdd(status, 1u);
}
__global__ __launch_bounds__(256) void uniq_resolve_lookup_kernel(const uint64_t* __restrict__ hash, uint64_t n, const UniqSlot* __restrict__ t, uint64_t mask,
                                                                  uint64_t* first_seen, uint8_t* keep, uint64_t base, const uint32_t* only_if = nullptr)
{
    if (only_if && *only_if == 0) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t v = uniq_find(t, mask, hash[i]);
        const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32), r = lo < hi ? lo : hi;
        first_seen[i] = r == 0xFFFFFFFFu ? UNIQ_EMPTY : base + r;           // (not found: only after a table overflow)
        if (keep) keep[i] = r == (uint32_t)i;
    }
}

// moves every (key, smallest index) entry of an old table into a bigger one
__global__ __launch_bounds__(256) void uniq_rehash_kernel(const UniqSlot* __restrict__ old, uint64_t oslots, UniqSlot* t, uint64_t mask)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < oslots; i += stride) {
        const UniqSlot e = uniq_peek(old + i);
        if (i + 1 == oslots) { if (e.val != UNIQ_EMPTY) atomicMin(&t[mask + 1].val, e.val); continue; }   // the EMPTY-key slot
        if (e.key != UNIQ_EMPTY) (void)uniq_fold(t, mask, e.key, e.val);
    }
}

// ---- multi-GPU exchange (circkit_amd/uniq.py, exchange="partition"): the key space is cut into `world` ranges, a key
// belongs to rank ((h >> 20) & 0x7FFFFFFF) % world (well-mixed middle bits of the XXH3 output).
constexpr uint32_t UNIQ_MAX_WORLD = 64;
__device__ __forceinline__ uint32_t uniq_owner(uint64_t h, uint32_t world) { return (uint32_t)((h >> 20) & 0x7FFFFFFFu) % world; }
// pass 1: keys per owner (one global atomic per workgroup and owner)
__global__ __launch_bounds__(256) void uniq_partition_count_kernel(const uint64_t* __restrict__ hash, uint64_t n, uint32_t world, unsigned long long* counts)
{
    __shared__ uint32_t hist[UNIQ_MAX_WORLD];
    if (threadIdx.x < UNIQ_MAX_WORLD) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&hist[uniq_owner(hash[i], world)], 1u);
    __syncthreads();
    if (threadIdx.x < world && hist[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}
// pass 2: rows[(pos)] = {hash, base + i} with the rows of one owner together (owners in rank order, any order inside),
// slot[i] = pos.  Each workgroup takes chunks of 256 * PER keys: a histogram of the chunk in LDS (the LDS atomic's return value
// is the key's rank inside its owner's share of the chunk), one global atomic per owner to reserve the chunk's rows, then every
// key its place.  PER = 4 with the keys RE-READ in the second phase (they are in the vector cache) instead of 16 with owner and
// rank of every key kept in registers: 131 VGPRs / 3 waves per SIMD -> under 40 / 8; the owners' base
// offsets are a prefix sum of the 64 counts done once per workgroup, not a loop per chunk.
__global__ __launch_bounds__(256) void uniq_partition_scatter_kernel(const uint64_t* __restrict__ hash, uint64_t n, uint64_t base, uint32_t world,
                                                                     const unsigned long long* __restrict__ counts, unsigned long long* cursor,
                                                                     uint64_t* rows, uint32_t* slot)
{
    __shared__ uint32_t hist[UNIQ_MAX_WORLD];
    __shared__ unsigned long long first[UNIQ_MAX_WORLD], start[UNIQ_MAX_WORLD];
    constexpr uint32_t PER = 4;
    const uint64_t chunk = 256ull * PER;
    if (threadIdx.x < UNIQ_MAX_WORLD) {                       // (one wave) exclusive prefix sum of the owners' totals
        unsigned long long v = threadIdx.x < world ? counts[threadIdx.x] : 0ull, incl = v;
        for (uint32_t d = 1; d < UNIQ_MAX_WORLD; d <<= 1) {
            const uint32_t lo = ck::shfl((uint32_t)incl, threadIdx.x - d), hi = ck::shfl((uint32_t)(incl >> 32), threadIdx.x - d);
            if (threadIdx.x >= d) incl += ((unsigned long long)hi << 32) | lo;
        }
        first[threadIdx.x] = incl - v;
    }
    for (uint64_t c0 = (uint64_t)blockIdx.x * chunk; c0 < n; c0 += (uint64_t)gridDim.x * chunk) {
        if (threadIdx.x < UNIQ_MAX_WORLD) hist[threadIdx.x] = 0;
        __syncthreads();
        uint32_t rank[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint64_t i = c0 + k * 256 + threadIdx.x;
            rank[k] = i < n ? atomicAdd(&hist[uniq_owner(hash[i], world)], 1u) : 0u;
        }
        __syncthreads();
        if (threadIdx.x < world)
            start[threadIdx.x] = first[threadIdx.x] + (hist[threadIdx.x] ? atomicAdd(&cursor[threadIdx.x], (unsigned long long)hist[threadIdx.x]) : 0ull);
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < PER; ++k) {
            const uint64_t i = c0 + k * 256 + threadIdx.x;
            if (i < n) {
                const uint64_t h = hash[i];
                const uint64_t pos = start[uniq_owner(h, world)] + rank[k];
                typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
                *reinterpret_cast<v2*>(rows + 2 * pos) = v2{ h, base + i };
                slot[i] = (uint32_t)pos;
            }
        }
        __syncthreads();
    }
}
// rows of {hash, global index}: fold them into the table / answer each with the smallest index seen for its hash
__global__ __launch_bounds__(256) void uniq_insert_rows_kernel(const uint64_t* __restrict__ rows, uint64_t n, UniqSlot* t, uint64_t mask, uint32_t* status)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const UniqSlot r = uniq_peek(reinterpret_cast<const UniqSlot*>(rows) + i);
        if (!uniq_fold(t, mask, r.key, r.val)) atomicAdd(status, 1u);
    }
}
__global__ __launch_bounds__(256) void uniq_lookup_rows_kernel(const uint64_t* __restrict__ rows, uint64_t n, const UniqSlot* __restrict__ t, uint64_t mask,
                                                               uint64_t* answers)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        answers[i] = uniq_find(t, mask, rows[2 * i]);
    }
}
// first_seen[i] = answers[slot[i]] (the answers arrive in row order)
__global__ __launch_bounds__(256) void uniq_gather_kernel(const uint64_t* __restrict__ answers, const uint32_t* __restrict__ slot, uint64_t n, uint64_t base,
                                                          uint64_t* first_seen, uint8_t* keep)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t r = answers[slot[i]];
        first_seen[i] = r;
        if (keep) keep[i] = r == base + i;
    }
}

// every slot = {EMPTY, EMPTY}: 16 bytes per thread and trip; also zeroes the overflow counter
__global__ __launch_bounds__(256) void uniq_clear_kernel(UniqSlot* t, uint64_t slots, uint32_t* overflow, const uint32_t* only_if = nullptr)
{
    if (only_if && *only_if == 0) return;
    typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
    if (overflow && blockIdx.x == 0 && threadIdx.x == 0) *overflow = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride)
        *reinterpret_cast<v2*>(t + i) = v2{ UNIQ_EMPTY, UNIQ_EMPTY };
}

// ---- circkit_uniq_resolve_device in LDS-sized buckets (round 4) --------------------------------------------------------------
// The open-addressing table in HBM costs every key a scattered 16-byte read and one or two memory-side atomics (10M keys:
// clear 0.05 + insert 0.48 + lookup 0.22 ms).  A shard that is resolved in ONE call needs no table that outlives it: the keys
// are partitioned by their top bits into buckets of ~1300..2600 keys (a counting pass, two small scans, a scatter of
// {hash, local index} rows -- no global atomic anywhere: every workgroup owns a contiguous range of the keys and its own column
// of the count matrix), and each bucket is resolved by one workgroup in a 4096-slot table in LDS (64-bit LDS compare-and-swap
// on the key, LDS atomic min on the index).  What stays scattered is the answer: first_seen[i] and keep[i] go to the record's
// own place.  A bucket with more than BKT_MAX keys (all records equal, say) raises a flag and the whole shard takes the HBM
// table behind it -- same answers; its three kernels return at once otherwise.  Scratch: the table's own memory (rows, count
// matrix, bucket totals and bases all fit the slots circkit_uniq_reset sizes for n keys).
#ifndef CK_BKT_NW
#define CK_BKT_NW 512
#endif
constexpr uint32_t BKT_NW = CK_BKT_NW, BKT_SLOTS = 4096, BKT_MAX = 3072, BKT_KEYS = 2600, BKT_MAX_LOG2 = 13;      // (mean bucket 1300..2600 keys; 2200 -- twice the buckets at 10M keys -- measured 1 % slower)
__device__ __forceinline__ uint32_t bkt_of(uint64_t h, uint32_t log2b) { return (uint32_t)(h >> (64 - log2b)); }
// counts[w][b] = keys of workgroup w's range in bucket b; also zeroes the fallback flag and the table-overflow counter
__global__ __launch_bounds__(1024) void uniq_bkt_count_kernel(const uint64_t* __restrict__ hash, uint64_t n, uint64_t per, uint32_t log2b, uint32_t* counts,
                                                              uint32_t* flag, uint32_t* overflow)
{
    extern __shared__ uint32_t bkt_lds[];
    const uint32_t B = 1u << log2b;
    for (uint32_t b = threadIdx.x; b < B; b += 1024) bkt_lds[b] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *flag = 0; *overflow = 0; }
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += 1024) atomicAdd(&bkt_lds[bkt_of(hash[i], log2b)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < B; b += 1024) counts[(uint64_t)blockIdx.x * B + b] = bkt_lds[b];
}
// per bucket: exclusive prefix of the counts over the workgroups (in place), the bucket's total.  A workgroup takes 64 buckets,
// sixteen threads per bucket with a 32nd of the column each (one thread per bucket walking all 512 counts: 65 us of latency)
__global__ __launch_bounds__(1024) void uniq_bkt_colscan_kernel(uint32_t* counts, uint32_t B, uint32_t* tot)
{
    __shared__ uint32_t seg[16][64];
    constexpr uint32_t PER = BKT_NW / 16;
    const uint32_t bl = threadIdx.x & 63, sg = threadIdx.x >> 6, b = blockIdx.x * 64 + bl;      // (B is a multiple of 64)
    uint32_t sum = 0;
    for (uint32_t w = sg * PER; w < (sg + 1) * PER; ++w) sum += counts[(uint64_t)w * B + b];
    seg[sg][bl] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t k = 0; k < sg; ++k) run += seg[k][bl];
    for (uint32_t w = sg * PER; w < (sg + 1) * PER; ++w) {
        const uint64_t k = (uint64_t)w * B + b;
        const uint32_t cnt = counts[k];
        counts[k] = run;
        run += cnt;
    }
    if (sg == 15) tot[b] = run;
}
// base[b] = first row of bucket b, base[B] = n (one workgroup; B <= 8192)
__global__ __launch_bounds__(1024) void uniq_bkt_basescan_kernel(const uint32_t* __restrict__ tot, uint32_t B, uint32_t* base)
{
    __shared__ uint32_t part[1024];
    const uint32_t items = (B + 1023) / 1024, b0 = threadIdx.x * items;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < items; ++k) if (b0 + k < B) sum += tot[b0 + k];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                   // inclusive scan of the partial sums
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t k = 0; k < items; ++k) if (b0 + k < B) { base[b0 + k] = run; run += tot[b0 + k]; }
    if (threadIdx.x == 1023) base[B] = part[1023];
}
// rows[base[b] + ...] = {hash, local index}; a workgroup's keys of bucket b start at base[b] + its prefix in the count matrix
__global__ __launch_bounds__(1024) void uniq_bkt_scatter_kernel(const uint64_t* __restrict__ hash, uint64_t n, uint64_t per, uint32_t log2b,
                                                                const uint32_t* __restrict__ counts, const uint32_t* __restrict__ base, uint64_t* rows,
                                                                uint64_t* first_seen, uint64_t base_index)
{
    // (every record starts out as its own first occurrence, written here in record order -- coalesced; the resolve kernel then
    // only has scattered answers for the records that are NOT: half the batch in BASELINE config 3, next to none in real inputs)
    extern __shared__ uint32_t bkt_lds[];
    const uint32_t B = 1u << log2b;
    for (uint32_t b = threadIdx.x; b < B; b += 1024) bkt_lds[b] = base[b] + counts[(uint64_t)blockIdx.x * B + b];
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
    typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
    constexpr int U = 4;                                    // keys in flight per thread (one at a time the loop is a chain of load latencies)
    uint64_t i = i0 + threadIdx.x;
    for (; i + (U - 1) * 1024 < i1; i += U * 1024) {
        uint64_t h[U];
#pragma unroll
        for (int u = 0; u < U; ++u) h[u] = hash[i + u * 1024];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t pos = atomicAdd(&bkt_lds[bkt_of(h[u], log2b)], 1u);
            *reinterpret_cast<v2*>(rows + 2 * (uint64_t)pos) = v2{ h[u], i + u * 1024 };
            first_seen[i + u * 1024] = base_index + i + u * 1024;
        }
    }
    for (; i < i1; i += 1024) {
        const uint64_t h = hash[i];
        const uint32_t pos = atomicAdd(&bkt_lds[bkt_of(h, log2b)], 1u);
        *reinterpret_cast<v2*>(rows + 2 * (uint64_t)pos) = v2{ h, i };
        first_seen[i] = base_index + i;
    }
}
// one workgroup per bucket: smallest local index per key in an LDS table, then every row's answer to its record's place
#ifndef BKT_RESOLVE_T
#define BKT_RESOLVE_T 1024     // threads per bucket: 48 KB of LDS allow two workgroups per CU -- at 1024 threads that is every wave slot (256: 12 of 32)
#endif
__global__ __launch_bounds__(BKT_RESOLVE_T) void uniq_bkt_resolve_kernel(const uint64_t* __restrict__ rows, const uint32_t* __restrict__ base, uint64_t base_index,
                                                               uint64_t* first_seen, uint8_t* keep, uint32_t* flag)
{
    __shared__ unsigned long long keys[BKT_SLOTS];
    __shared__ uint32_t idx[BKT_SLOTS], special;
    const uint32_t r0 = base[blockIdx.x], cnt = base[blockIdx.x + 1] - r0;
    if (cnt == 0) return;
    if (cnt > BKT_MAX) { if (threadIdx.x == 0) atomicExch(flag, 1u); return; }      // the HBM table has this shard (every record of it)
    for (uint32_t s = threadIdx.x; s < BKT_SLOTS; s += BKT_RESOLVE_T) { keys[s] = UNIQ_EMPTY; idx[s] = 0xFFFFFFFFu; }
    if (threadIdx.x == 0) special = 0xFFFFFFFFu;
    __syncthreads();
    // a thread's rows stay in registers between the two passes (cnt <= BKT_MAX = 3 x 1024)
    constexpr uint32_t RPT = (BKT_MAX + BKT_RESOLVE_T - 1) / BKT_RESOLVE_T;
    uint64_t hk[RPT];
    uint32_t ik[RPT];
#pragma unroll
    for (uint32_t k = 0; k < RPT; ++k) {
        const uint32_t r = threadIdx.x + k * BKT_RESOLVE_T;
        hk[k] = 0; ik[k] = 0xFFFFFFFFu;
        if (r < cnt) { const UniqSlot row = uniq_peek(reinterpret_cast<const UniqSlot*>(rows) + r0 + r); hk[k] = row.key; ik[k] = (uint32_t)row.val; }
    }
#pragma unroll
    for (uint32_t k = 0; k < RPT; ++k) {
        if (ik[k] == 0xFFFFFFFFu) continue;
        const uint64_t h = hk[k];
        if (h == UNIQ_EMPTY) { atomicMin(&special, ik[k]); continue; }
        uint32_t s = (uint32_t)(h ^ (h >> 29)) & (BKT_SLOTS - 1);
        for (;;) {
            const unsigned long long old = atomicCAS(&keys[s], (unsigned long long)UNIQ_EMPTY, (unsigned long long)h);
            if (old == UNIQ_EMPTY || old == h) { atomicMin(&idx[s], ik[k]); break; }
            s = (s + 1) & (BKT_SLOTS - 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < RPT; ++k) {
        if (ik[k] == 0xFFFFFFFFu) continue;
        const uint64_t h = hk[k];
        uint32_t m;
        if (h == UNIQ_EMPTY) m = special;
        else {
            uint32_t s = (uint32_t)(h ^ (h >> 29)) & (BKT_SLOTS - 1);
            while (keys[s] != h) s = (s + 1) & (BKT_SLOTS - 1);
            m = idx[s];
        }
        if (m != ik[k]) first_seen[ik[k]] = base_index + m;     // (the one scattered store, for records that repeat an earlier one; keep[] follows, coalesced)
    }
}
// keep[i] = 1 iff record i is the first with its hash
__global__ __launch_bounds__(256) void uniq_keep_kernel(const uint64_t* __restrict__ first_seen, uint64_t n, uint64_t base, uint8_t* keep, const uint32_t* skip_if)
{
    if (skip_if && *skip_if != 0) return;                   // (the fallback writes its own)
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) keep[i] = first_seen[i] == base + i;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
#ifndef CK_UNIQ_BPC
#define CK_UNIQ_BPC 8        // workgroups of 256 threads per CU for the table kernels (one key per thread and trip)
#endif
#ifndef CK_UNIQ_LOAD_PCT
#define CK_UNIQ_LOAD_PCT 70       // circkit_uniq_reset sizes the table for at most this load with `expected_keys` distinct keys
#endif
constexpr int N_CU = 256;                                // (as in canon_config.h, by which the canonicalize unit sizes its own grids)
constexpr unsigned UNIQ_GRID = N_CU * CK_UNIQ_BPC;       // the table kernels' grid, by 256 threads

// the words the kernels report through and the partition step's scatter cursors: one small device allocation, zeroed when made
struct UniqWords {
    uint32_t overflow;                                   // keys that found no slot since the last reset (circkit_uniq_status)
    uint32_t bucket_flag;                                // the bucketed resolve: a bucket was too big, the HBM table has the shard
    unsigned long long cursor[UNIQ_MAX_WORLD];
};

struct UniqState {
    ck_buf<UniqSlot> d_table;            // [mask + 2]
    uint64_t mask = 0, count = 0;        // slots - 1; upper bound of the keys folded in so far
    bool local = false;                  // the table holds circkit_uniq_resolve_device's split local values
    bool lost = false;                   // a rehash failed half-way: the stream's earlier batches are gone -- every uniq call fails until circkit_uniq_reset
    ck_buf<UniqWords> d_words;
    // circkit_uniq_first_seen's staging: the batch's keys and their answers
    ck_buf<uint64_t> d_keys, d_answers;
};

// Every entry point that touches the state starts here: sets the ctx's device and hands out its uniq state, made on first use
// (the words zeroed on the ctx stream, in order with every later use of them).
int uniq_state(circkit_ctx* c, UniqState** out)
{
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    UniqState* S = *out = ck_unit_state<UniqState>(c, CK_UNIT_UNIQ);
    if (!S->d_words) {
        const int rc = S->d_words.grow(c, 1);
        if (rc) return rc;
        const hipError_t e = hipMemsetAsync(S->d_words, 0, sizeof(UniqWords), ck_ctx_stream(c));
        if (e != hipSuccess) { S->d_words.release(); return ck_fail(c, CIRCKIT_ERR_HIP, "hipMemsetAsync failed: %s", hipGetErrorString(e)); }
    }
    return CIRCKIT_OK;
}

// the table calls' precondition: a table made by circkit_uniq_reset that no resolve has taken over since
int uniq_table_ready(circkit_ctx* c, UniqState** out)
{
    const int rc = uniq_state(c, out);
    if (rc) return rc;
    if (!(*out)->d_table || (*out)->local)
        return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "circkit_uniq_reset has not been called (since the last circkit_uniq_resolve_device)");
    return CIRCKIT_OK;
}

// the table sized (allocated) for `expected_keys` distinct keys at CK_UNIQ_LOAD_PCT; contents untouched
int uniq_size(circkit_ctx* c, UniqState* S, uint64_t expected_keys)
{
    uint64_t cap = 1024;
    while (cap * CK_UNIQ_LOAD_PCT < expected_keys * 100) cap <<= 1;
    if (cap - 1 != S->mask || !S->d_table) {
        S->mask = 0;
        S->d_table.release();            // another size, not only a larger one
        int rc;
        if ((rc = S->d_table.grow(c, cap + 1))) return rc;
        S->mask = cap - 1;
    }
    return CIRCKIT_OK;
}

}  // namespace

// ck_ctx.h's: the overflow word for a unit that keeps the count of its own resolve
int ck_uniq_overflow_word(circkit_ctx* c, const uint32_t** out)
{
    UniqState* S;
    const int rc = uniq_state(c, &S);
    if (rc) return rc;
    *out = &S->d_words->overflow;
    return CIRCKIT_OK;
}

extern "C" {

int circkit_uniq_reset(circkit_ctx* c, uint64_t expected_keys)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    UniqState* S;
    int rc = uniq_state(c, &S);
    if (rc || (rc = uniq_size(c, S, expected_keys))) return rc;
    const uint64_t cap = S->mask + 1;
    hipLaunchKernelGGL(uniq_clear_kernel, dim3(N_CU * 8), dim3(256), 0, ck_ctx_stream(c), S->d_table, cap + 1, &S->d_words->overflow);
    CK_HIP(c, hipGetLastError());
    S->count = 0;
    S->local = false;
    S->lost = false;
    return CIRCKIT_OK;
}

// Host-buffer form for streaming hosts (the CLI): folds this batch's hashes into the table, growing (and
// rehashing) it as the stream gets longer, and returns the winners.  Synchronizes.
int circkit_uniq_first_seen(circkit_ctx* c, const uint64_t* hash, uint64_t n, uint64_t base_index, uint64_t* first_seen)
{
    if (!c || (n && (!hash || !first_seen))) return CIRCKIT_ERR_INVALID_ARG;
    if (n == 0) return CIRCKIT_OK;
    UniqState* S;
    int rc = uniq_state(c, &S);
    if (rc) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if (S->lost)
        return ck_fail(c, CIRCKIT_ERR_HIP, "the uniq table was lost in a failed rehash: the earlier batches of this stream are gone "
                       "(circkit_uniq_reset starts a new one)");
    if (S->local) { const int rc0 = circkit_uniq_reset(c, n); if (rc0) return rc0; }      // a resolve result is not a stream's table
    if (!S->d_table || (S->count + n) * 2 > S->mask + 1) {
        uint64_t cap = 1 << 16;
        while (cap < 4 * (S->count + n)) cap <<= 1;
        UniqSlot* nt = nullptr;
        CK_HIP(c, hipMalloc(&nt, (cap + 1) * sizeof(UniqSlot)));
        hipLaunchKernelGGL(uniq_clear_kernel, dim3(N_CU * 8), dim3(256), 0, st, nt, cap + 1, (uint32_t*)nullptr);
        if (S->d_table) {
            hipLaunchKernelGGL(uniq_rehash_kernel, dim3(N_CU * 8), dim3(256), 0, st, (const UniqSlot*)S->d_table, S->mask + 2, nt, cap - 1);
            hipError_t e = hipStreamSynchronize(st);
            if (e == hipSuccess && getenv("CIRCKIT_TEST_FAIL_REHASH")) e = hipErrorUnknown;      // fault injection (tests/test_gpu_parity.py)
            S->d_table.release();
            if (e != hipSuccess) {
                // the old table is gone and the new one holds who knows what: not a state to go on from silently -- every
                // later call fails until the caller starts over with circkit_uniq_reset
                (void)hipFree(nt);
                S->mask = 0; S->count = 0; S->lost = true;
                return ck_fail(c, CIRCKIT_ERR_HIP, "uniq table rehash failed: %s", hipGetErrorString(e));
            }
        } else {
            CK_HIP(c, hipMemsetAsync(&S->d_words->overflow, 0, 4, st));
        }
        S->d_table.adopt(nt, cap + 1); S->mask = cap - 1;
    }
    if (n > S->d_keys.cap || n > S->d_answers.cap) {
        const uint64_t nk = n + n / 8 + 1024;
        if ((rc = S->d_keys.grow(c, nk))) return rc;
        if ((rc = S->d_answers.grow(c, nk))) return rc;
    }
    CK_HIP(c, hipMemcpyAsync(S->d_keys, hash, n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(uniq_insert_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, (const uint64_t*)S->d_keys, (const uint64_t*)nullptr, n, base_index,
                       S->d_table, S->mask, &S->d_words->overflow);
    hipLaunchKernelGGL(uniq_lookup_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, (const uint64_t*)S->d_keys, n, (const UniqSlot*)S->d_table,
                       S->mask, S->d_answers, (uint8_t*)nullptr, (uint64_t)0);
    CK_HIP(c, hipGetLastError());
    CK_HIP(c, hipMemcpyAsync(first_seen, S->d_answers, n * 8, hipMemcpyDeviceToHost, st));
    CK_HIP(c, hipStreamSynchronize(st));
    S->count += n;
    return CIRCKIT_OK;
}

int circkit_uniq_insert_device(circkit_ctx* c, const uint64_t* d_hash, uint64_t n, uint64_t base_index)
{
    if (!c || (n && !d_hash)) return CIRCKIT_ERR_INVALID_ARG;
    UniqState* S;
    const int rc = uniq_table_ready(c, &S);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_insert_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_hash, (const uint64_t*)nullptr, n, base_index,
                       S->d_table, S->mask, &S->d_words->overflow);
    CK_HIP(c, hipGetLastError());
    S->count += n;
    return CIRCKIT_OK;
}

int circkit_uniq_insert_pairs_device(circkit_ctx* c, const uint64_t* d_hash, const uint64_t* d_index, uint64_t n)
{
    if (!c || (n && (!d_hash || !d_index))) return CIRCKIT_ERR_INVALID_ARG;
    UniqState* S;
    const int rc = uniq_table_ready(c, &S);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_insert_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_hash, d_index, n, (uint64_t)0, S->d_table,
                       S->mask, &S->d_words->overflow);
    CK_HIP(c, hipGetLastError());
    S->count += n;
    return CIRCKIT_OK;
}

// Enqueues the lookups; a table overflow of the inserts before it is reported by circkit_uniq_status (or by the next
// synchronising uniq call) -- this call itself does not wait for the GPU.
int circkit_uniq_lookup_device(circkit_ctx* c, const uint64_t* d_hash, uint64_t n, uint64_t* d_first_seen)
{
    if (!c || (n && (!d_hash || !d_first_seen))) return CIRCKIT_ERR_INVALID_ARG;
    UniqState* S;
    const int rc = uniq_table_ready(c, &S);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_lookup_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_hash, n, (const UniqSlot*)S->d_table, S->mask, d_first_seen,
                       (uint8_t*)nullptr, (uint64_t)0);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// ---- the multi-GPU exchange's device steps (circkit_amd/uniq.py; include/circkit.h)
int circkit_uniq_partition_device(circkit_ctx* c, const uint64_t* d_hash, uint64_t n, uint64_t base_index, uint32_t world, uint64_t* d_rows,
                                  uint64_t* d_counts, uint32_t* d_slot)
{
    if (!c || !d_counts || world == 0 || world > UNIQ_MAX_WORLD || (n && (!d_hash || !d_rows || !d_slot))) return CIRCKIT_ERR_INVALID_ARG;
    if (n >= 0xFFFFFFFFull) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "circkit_uniq_partition_device: n must be < 2^32 - 1");
    if ((uintptr_t)d_rows & 15) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_rows must be 16-byte aligned");
    UniqState* S;
    const int rc = uniq_state(c, &S);
    if (rc) return rc;
    hipStream_t st = ck_ctx_stream(c);
    CK_HIP(c, hipMemsetAsync(d_counts, 0, world * sizeof(uint64_t), st));
    CK_HIP(c, hipMemsetAsync(S->d_words->cursor, 0, sizeof S->d_words->cursor, st));      // the scatter's cursors
    if (n == 0) return CIRCKIT_OK;
    hipLaunchKernelGGL(uniq_partition_count_kernel, dim3(N_CU * 8), dim3(256), 0, st, d_hash, n, world, (unsigned long long*)d_counts);
    hipLaunchKernelGGL(uniq_partition_scatter_kernel, dim3(N_CU * 8), dim3(256), 0, st, d_hash, n, base_index, world,
                       (const unsigned long long*)d_counts, S->d_words->cursor, d_rows, d_slot);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int circkit_uniq_insert_rows_device(circkit_ctx* c, const uint64_t* d_rows, uint64_t n)
{
    if (!c || (n && !d_rows)) return CIRCKIT_ERR_INVALID_ARG;
    if ((uintptr_t)d_rows & 15) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_rows must be 16-byte aligned");
    UniqState* S;
    const int rc = uniq_table_ready(c, &S);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_insert_rows_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_rows, n, S->d_table, S->mask, &S->d_words->overflow);
    CK_HIP(c, hipGetLastError());
    S->count += n;
    return CIRCKIT_OK;
}

int circkit_uniq_lookup_rows_device(circkit_ctx* c, const uint64_t* d_rows, uint64_t n, uint64_t* d_answers)
{
    if (!c || (n && (!d_rows || !d_answers))) return CIRCKIT_ERR_INVALID_ARG;
    if ((uintptr_t)d_rows & 15) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_rows must be 16-byte aligned");
    UniqState* S;
    const int rc = uniq_table_ready(c, &S);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_lookup_rows_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_rows, n, (const UniqSlot*)S->d_table, S->mask, d_answers);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int circkit_uniq_gather_device(circkit_ctx* c, const uint64_t* d_answers, const uint32_t* d_slot, uint64_t n, uint64_t base_index, uint64_t* d_first_seen,
                               uint8_t* d_keep)
{
    if (!c || (n && (!d_answers || !d_slot || !d_first_seen))) return CIRCKIT_ERR_INVALID_ARG;
    if (n == 0) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    hipLaunchKernelGGL(uniq_gather_kernel, dim3(UNIQ_GRID), dim3(256), 0, ck_ctx_stream(c), d_answers, d_slot, n, base_index, d_first_seen, d_keep);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// One shard, one call: table reset, insert, lookup and the keep flags -- the whole first-seen resolution of a batch whose
// record i has global index base_index + i (what `circkit uniq` decides per record on one GPU).  Only enqueues work.
int circkit_uniq_resolve_device(circkit_ctx* c, const uint64_t* d_hash, uint64_t n, uint64_t base_index, uint64_t* d_first_seen, uint8_t* d_keep)
{
    if (!c || (n && (!d_hash || !d_first_seen))) return CIRCKIT_ERR_INVALID_ARG;
    if (n >= 0xFFFFFFFFull) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "circkit_uniq_resolve_device: n must be < 2^32 - 1");     // before the table is touched
    UniqState* S;
    int rc = uniq_state(c, &S);
    if (rc) return rc;
    hipStream_t st = ck_ctx_stream(c);
    uint32_t* overflow = &S->d_words->overflow;
#ifndef CK_BKT_KEYS
#define CK_BKT_KEYS BKT_KEYS
#endif
#ifndef CK_UNIQ_BUCKET_MIN
#define CK_UNIQ_BUCKET_MIN (1u << 19)      // shards below this take the HBM table directly (the bucketed path is five launches)
#endif
    static const bool no_buckets = getenv("CIRCKIT_UNIQ_NO_BUCKETS") != nullptr;
    // (shards beyond 2600 x 8192 = 21M keys would overfill their buckets -- the count / scatter histograms hold 8192 bins in LDS --
    // and take the HBM table directly, like the small ones)
    if (n >= CK_UNIQ_BUCKET_MIN && n <= ((uint64_t)CK_BKT_KEYS << BKT_MAX_LOG2) && !no_buckets) {
        // LDS-sized buckets (see uniq_bkt_*_kernel); the table's memory is the scratch, the table itself only the fallback
        rc = uniq_size(c, S, n);
        if (rc) return rc;
        uint32_t log2b = 6;
        while (log2b < BKT_MAX_LOG2 && ((uint64_t)CK_BKT_KEYS << log2b) < n) ++log2b;
        const uint32_t B = 1u << log2b;
        const uint64_t per = (n + BKT_NW - 1) / BKT_NW;
        uint8_t* scratch = reinterpret_cast<uint8_t*>(S->d_table.p);
        uint64_t* rows = reinterpret_cast<uint64_t*>(scratch);
        uint32_t* counts = reinterpret_cast<uint32_t*>(scratch + ((n * 16 + 255) & ~255ull));
        uint32_t* tot = counts + (uint64_t)BKT_NW * B;
        uint32_t* base = tot + B;
        if ((uint64_t)(reinterpret_cast<uint8_t*>(base + B + 1) - scratch) > (S->mask + 2) * sizeof(UniqSlot))
            return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "internal: bucket scratch does not fit the table");
        uint32_t* flag = &S->d_words->bucket_flag;
        hipLaunchKernelGGL(uniq_bkt_count_kernel, dim3(BKT_NW), dim3(1024), B * 4, st, d_hash, n, per, log2b, counts, flag, overflow);
        hipLaunchKernelGGL(uniq_bkt_colscan_kernel, dim3(B / 64), dim3(1024), 0, st, counts, B, tot);
        hipLaunchKernelGGL(uniq_bkt_basescan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)tot, B, base);
        hipLaunchKernelGGL(uniq_bkt_scatter_kernel, dim3(BKT_NW), dim3(1024), B * 4, st, d_hash, n, per, log2b, (const uint32_t*)counts, (const uint32_t*)base, rows, d_first_seen, base_index);
        hipLaunchKernelGGL(uniq_bkt_resolve_kernel, dim3(B), dim3(BKT_RESOLVE_T), 0, st, (const uint64_t*)rows, (const uint32_t*)base, base_index, d_first_seen, d_keep, flag);
        if (d_keep) hipLaunchKernelGGL(uniq_keep_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, (const uint64_t*)d_first_seen, n, base_index, d_keep, (const uint32_t*)flag);
        // the fallback (a bucket beyond BKT_MAX keys): the HBM table over the whole shard; three launches that return at once otherwise
        hipLaunchKernelGGL(uniq_clear_kernel, dim3(N_CU * 8), dim3(256), 0, st, S->d_table, S->mask + 2, (uint32_t*)nullptr, (const uint32_t*)flag);
        hipLaunchKernelGGL(uniq_resolve_insert_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, d_hash, n, S->d_table, S->mask, overflow, (const uint32_t*)flag);
        hipLaunchKernelGGL(uniq_resolve_lookup_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, d_hash, n, (const UniqSlot*)S->d_table, S->mask,
                           d_first_seen, d_keep, base_index, (const uint32_t*)flag);
        CK_HIP(c, hipGetLastError());
        S->local = true;
        S->count = n;
        S->lost = false;
        return CIRCKIT_OK;
    }
    rc = circkit_uniq_reset(c, n);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(uniq_resolve_insert_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, d_hash, n, S->d_table, S->mask, overflow);
    hipLaunchKernelGGL(uniq_resolve_lookup_kernel, dim3(UNIQ_GRID), dim3(256), 0, st, d_hash, n, (const UniqSlot*)S->d_table, S->mask,
                       d_first_seen, d_keep, base_index);
    CK_HIP(c, hipGetLastError());
    S->local = true;       // the table now holds split local values: circkit_uniq_reset before any other use
    S->count = n;
    // (Clearing the table for the NEXT call here, on a side stream behind the lookup, so that the 268 MB of stores run under
    // the next batch's hash kernel, was tried: 5.21 -> 5.18 ms, inside the noise -- that kernel has no bandwidth to spare.)
    return CIRCKIT_OK;
}

int circkit_uniq_status(circkit_ctx* c, uint32_t* n_overflowed)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    UniqState* S;
    const int rc = uniq_state(c, &S);
    if (rc) return rc;
    uint32_t overflow = 0;
    CK_HIP(c, hipMemcpyAsync(&overflow, &S->d_words->overflow, 4, hipMemcpyDeviceToHost, ck_ctx_stream(c)));
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    if (n_overflowed) *n_overflowed = overflow;
    if (overflow) return ck_fail(c, CIRCKIT_ERR_OOM, "uniq table overflow: %u key(s) found no slot (more distinct keys than circkit_uniq_reset sized it for)", overflow);
    return CIRCKIT_OK;
}

}  // extern "C"
