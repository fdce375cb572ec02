// ck_scan.h -- the prefix scan of the batch units, once: a workgroup scan over LDS (Hillis-Steele doubling, three barriers a step)
// and the three tile-level bodies of the device scan built on it (tile sums, one workgroup that makes the sums exclusive WG at a
// time, the base of each thread within its tile).  The __global__ kernels stay in their units, under their names and launch
// bounds: each declares its LDS array, passes its thread and workgroup index and keeps its own thread-0 epilogue.
// Written against wave_prims.h only (CK_DEV, ck::block_barrier): every routine takes the thread's index `tid`, the tile and the
// LDS array from its caller, so the CPU fiber harness of tests/emu/ runs this source unchanged (tid = 64 * wave_in_block() +
// lane_id()).  Every routine is called by all WG threads of the workgroup in uniform control flow: each holds barriers.
//
// An operation Op carries the element type T, identity() and combine(earlier, later).  The operand order is part of the
// contract: combine need not be commutative (ck_fasta::next_state is not), only associative, and `earlier` is always the
// operand made of the elements in front.  (CK_DEV makes the members static on the host and plain members on the device: they
// are called on a temporary, Op().combine(a, b), which is right for both.)
#pragma once
#include <stdint.h>
#include "wave_prims.h"

namespace ck_scan {

// a + b, or ~0 where that does not fit: a scan of lengths stays monotone whatever lengths its items name, and a batch whose
// total does not fit 64 bits has the total ~0, which no capacity holds
CK_DEV uint64_t sat_add(uint64_t a, uint64_t b)
{
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}

struct Add {                                             // wrapping
    typedef uint64_t T;
    CK_DEV T identity() { return 0; }
    CK_DEV T combine(T earlier, T later) { return earlier + later; }
};
struct SatAdd {
    typedef uint64_t T;
    CK_DEV T identity() { return 0; }
    CK_DEV T combine(T earlier, T later) { return sat_add(earlier, later); }
};

// Exclusive scan over the workgroup: returns what the threads in front of `tid` combine to, *total = what all WG combine to
// (to every thread).  lds holds WG elements and is free again on return: the last barrier is behind the last read.
template <int WG, typename Op>
CK_DEV typename Op::T block_scan(uint32_t tid, typename Op::T v, typename Op::T* lds, typename Op::T* total)
{
    typedef typename Op::T T;
    lds[tid] = v;
    ck::block_barrier();
    for (int d = 1; d < WG; d <<= 1) {
        const T prev = tid >= (uint32_t)d ? lds[tid - d] : Op().identity();
        ck::block_barrier();
        lds[tid] = Op().combine(prev, lds[tid]);
        ck::block_barrier();
    }
    const T before = tid ? lds[tid - 1] : Op().identity();
    *total = lds[WG - 1];
    ck::block_barrier();
    return before;
}

// ---- the device scan over n items in tiles of WG * ITEMS; thread tid of tile `tile` owns ITEMS in a row ----
// The items are 64-bit words a[0..n) and elem(word) is the element a word stands for: the word itself for a scan of lengths,
// the compact's (written, bytes) pair.

// first kernel: what the items of the tile combine to (to every thread; one of them stores it as sums[tile])
template <int WG, int ITEMS, typename Op, typename Elem>
CK_DEV typename Op::T tile_sum(uint32_t tid, uint64_t tile, const uint64_t* a, uint64_t n, Elem elem, typename Op::T* lds)
{
    typedef typename Op::T T;
    const uint64_t t0 = tile * (uint64_t)(WG * ITEMS) + (uint64_t)tid * ITEMS;
    T v = Op().identity(), total;
    for (int k = 0; k < ITEMS; ++k) if (t0 + k < n) v = Op().combine(v, elem(a[t0 + k]));
    block_scan<WG, Op>(tid, v, lds, &total);
    return total;
}

// middle kernel, ONE workgroup: sums[0..n_tiles) become exclusive in rounds of WG; returns the grand total (to every thread)
template <int WG, typename Op>
CK_DEV typename Op::T sums_exclusive(uint32_t tid, typename Op::T* sums, uint64_t n_tiles, typename Op::T* lds)
{
    typedef typename Op::T T;
    T carry = Op().identity();
    for (uint64_t b = 0; b < n_tiles; b += WG) {
        const uint64_t idx = b + tid;
        T chunk;
        const T before = block_scan<WG, Op>(tid, idx < n_tiles ? sums[idx] : Op().identity(), lds, &chunk);
        if (idx < n_tiles) sums[idx] = Op().combine(carry, before);
        carry = Op().combine(carry, chunk);
    }
    return carry;
}

// last kernel: what everything in front of the thread's first item combines to (sums is exclusive by now); w[k] = the thread's
// k-th word, 0 beyond n, and elem(0) must be the identity.  The words are loaded first and turned into elements afterwards: an
// elem() inside the guarded load makes every load wait for its own data, where these ITEMS loads are in flight together.
template <int WG, int ITEMS, typename Op, typename Elem>
CK_DEV typename Op::T tile_base(uint32_t tid, uint64_t tile, const uint64_t* a, uint64_t n, Elem elem, const typename Op::T* sums,
                                typename Op::T* lds, uint64_t* w)
{
    typedef typename Op::T T;
    const uint64_t t0 = tile * (uint64_t)(WG * ITEMS) + (uint64_t)tid * ITEMS;
    for (int k = 0; k < ITEMS; ++k) w[k] = t0 + k < n ? a[t0 + k] : 0;
    T v = Op().identity(), total;
    for (int k = 0; k < ITEMS; ++k) v = Op().combine(v, elem(w[k]));
    return Op().combine(sums[tile], block_scan<WG, Op>(tid, v, lds, &total));
}

// ... and the last kernel of a scan of 64-bit lengths (the element is the word) in place: a[i] = item i's length becomes where
// item i ends
template <int WG, int ITEMS, typename Op>
CK_DEV void apply_ends(uint32_t tid, uint64_t tile, uint64_t* a, uint64_t n, const uint64_t* sums, uint64_t* lds)
{
    const uint64_t t0 = tile * (uint64_t)(WG * ITEMS) + (uint64_t)tid * ITEMS;
    uint64_t w[ITEMS];
    uint64_t run = tile_base<WG, ITEMS, Op>(tid, tile, a, n, [](uint64_t x) { return x; }, sums, lds, w);
    for (int k = 0; k < ITEMS; ++k) {
        run = Op().combine(run, w[k]);
        if (t0 + k < n) a[t0 + k] = run;
    }
}

}  // namespace ck_scan
