// prealign.h -- the rotation and strand that put one circular record onto another: the "pre-alignment of circular records" section
// of include/circkit.h, which is the definition.  Two records that share a k-mer of a sketch bin each know where it starts and on
// which strand its canonical form lies (the anchors of sketch.h); every such bin votes for a (strand, start) of the second record,
// and the most frequent vote wins.  Written against wave_prims.h only (and sketch.h for EMPTY and the 64-bit add); every collective
// (ballot, shfl, wave_sync, wave_sum_u64) sits in wave-uniform control flow, so the CPU fiber harness of tests/emu/ runs this
// source unchanged.
//
//   pair_wave    one pair by one wave.  A lane takes two bins a step (16 bytes of either row, 8 of either anchor row) and writes
//                their keys, NONE where the bin does not match, to the wave's slice of LDS (one word a bin); the keys are sorted
//                in place (a bitonic network, NONE last); a lane that finds the first key of a run looks for the run's end by
//                bisection; the wave maximum of (length << 32) | ~key is the longest run, the smallest key among equals.
//   labels_lane  one lane per record: the pair (labels[i], i)
// Anchors enter arithmetic only: nothing is dereferenced through them, and start < n_b holds for any anchor values.
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "sketch.h"

namespace ck_prealign {

constexpr uint32_t NONE = 0xFFFFFFFFu;                   // an anchor that does not exist, a bin that does not vote
constexpr uint32_t PREALIGN_WAVES = 4;                   // waves per workgroup, each with 1 << log2_bins words of LDS
constexpr uint32_t WINDOW_BYTES = 24;                    // sizeof(circkit_window)
enum { T_ALIGNED, T_INVALID, T_WORDS };                  // the totals of a pairs call, in device memory

#ifdef CK_WAVE_PRIMS_OVERRIDE
CK_DEV void load8(const uint8_t* p, uint32_t& a, uint32_t& b) { memcpy(&a, p, 4); memcpy(&b, p + 4, 4); }
#else
CK_DEV void load8(const uint8_t* p, uint32_t& a, uint32_t& b)
{
    typedef uint32_t v2 __attribute__((ext_vector_type(2), aligned(4)));
    const v2 v = *reinterpret_cast<const v2*>(p);
    a = v.x; b = v.y;
}
#endif

struct Prealign {
    const uint64_t* rows;            // n_records << log2_bins
    const uint32_t* anchors;         // n_records << log2_bins
    const uint64_t* offsets;         // n_records + 1
    uint64_t n_records;
    uint32_t k, log2_bins, min_votes;
    const uint32_t* pairs;           // (a, b) * n_pairs
    uint64_t n_pairs;
    uint8_t* windows;                // n_pairs circkit_window, 8-byte aligned
    uint32_t* scores;                // (votes, matches) * n_pairs
    uint64_t* totals;                // T_WORDS
};

// The vote of one matching bin: anchors aa of record a and ab of record b (n_b symbols, 0 < n_b < 2^31).
CK_DEV uint32_t vote_key(uint32_t aa, uint32_t ab, uint32_t n_b, uint32_t k)
{
    const uint32_t pa = aa >> 1, s = (aa ^ ab) & 1u;
    uint32_t pb = (ab >> 1) % n_b;
    if (s) {                                                             // the same k-mer's start on revcomp(b): (n_b - pb - k) mod n_b
        const uint32_t t = (pb + k % n_b) % n_b;                         // (both < n_b < 2^31: the sum fits)
        pb = t ? n_b - t : 0;
    }
    const uint32_t qa = pa % n_b;
    const uint32_t start = pb >= qa ? pb - qa : pb + n_b - qa;
    return (s << 31) | start;
}

// the keys[0 .. bins) of the wave's slice in ascending order; bins is a power of two >= 16
CK_DEV void sort_keys(uint32_t* keys, uint32_t bins)
{
    const uint32_t lane = ck::lane_id();
    for (uint32_t size = 2; size <= bins; size <<= 1) {
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t t = lane; t < bins / 2; t += 64) {
                const uint32_t i = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), j = i | stride;      // the t-th comparator
                const uint32_t x = keys[i], y = keys[j];
                const bool up = (i & size) == 0;
                if ((x > y) == up) { keys[i] = y; keys[j] = x; }
            }
            ck::wave_sync();
        }
    }
}

CK_DEV uint64_t wave_max_u64(uint64_t v)
{
    for (uint32_t m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = ck::shfl((uint32_t)v, ck::lane_id() ^ m), hi = ck::shfl((uint32_t)(v >> 32), ck::lane_id() ^ m);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

CK_DEV void store_window(uint8_t* w, uint64_t length, uint32_t record, uint32_t start, uint32_t strand)
{
    ck::store16(w, ck::u32x4{ (uint32_t)length, (uint32_t)(length >> 32), record, start });
    ck::store8(w + 16, strand, 0u);
}

// One pair by one wave, keys: the wave's 1 << log2_bins words of LDS.  *aligned: whether the votes reached min_votes.  Returns
// whether the pair is invalid (both wave-uniform).
CK_DEV bool pair_wave(const Prealign& P, uint64_t pair, uint32_t* keys, bool* aligned)
{
    const uint32_t lane = ck::lane_id(), bins = 1u << P.log2_bins;
    const uint64_t a = P.pairs[2 * pair], b = P.pairs[2 * pair + 1];
    uint8_t* w = P.windows + pair * WINDOW_BYTES;
    *aligned = false;
    if (a >= P.n_records || b >= P.n_records) {
        if (lane == 0) {
            store_window(w, 0, (uint32_t)b, 0, 0);
            ck::store8((uint8_t*)(P.scores + 2 * pair), 0u, 0u);
        }
        return true;
    }
    const uint64_t len_b = P.offsets[b + 1] - P.offsets[b];
    const bool votes_count = len_b != 0 && len_b < ck_sketch::TOO_LONG;  // a length of 0, or of 2^31 or more, never enters the modulus
    const uint32_t n_b = votes_count ? (uint32_t)len_b : 1u;
    const uint64_t *ra = P.rows + (a << P.log2_bins), *rb = P.rows + (b << P.log2_bins);
    const uint32_t *aa = P.anchors + (a << P.log2_bins), *ab = P.anchors + (b << P.log2_bins);
    uint32_t matches = 0;
    for (uint32_t b0 = 0; b0 < bins; b0 += 128) {
        const uint32_t at = b0 + 2 * lane;                               // bins is a multiple of 16: with at, at + 1 is a bin too
        bool m0 = false, m1 = false;
        if (at < bins) {
            const ck::u32x4 x = ck::load16((const uint8_t*)(ra + at)), y = ck::load16((const uint8_t*)(rb + at));
            uint32_t a0, a1, c0, c1;
            load8((const uint8_t*)(aa + at), a0, a1);
            load8((const uint8_t*)(ab + at), c0, c1);
            m0 = x.x == y.x && x.y == y.y && (x.x & x.y) != ~0u && a0 != NONE && c0 != NONE;
            m1 = x.z == y.z && x.w == y.w && (x.z & x.w) != ~0u && a1 != NONE && c1 != NONE;
            keys[at] = m0 && votes_count ? vote_key(a0, c0, n_b, P.k) : NONE;
            keys[at + 1] = m1 && votes_count ? vote_key(a1, c1, n_b, P.k) : NONE;
        }
        matches += (uint32_t)ck::popc64(ck::ballot(m0)) + (uint32_t)ck::popc64(ck::ballot(m1));
    }
    ck::wave_sync();
    sort_keys(keys, bins);
    uint64_t best = 0;
    for (uint32_t i = lane; i < bins; i += 64) {
        const uint32_t v = keys[i];
        if (v == NONE || (i && keys[i - 1] == v)) continue;             // not the first of a run
        uint32_t lo = i, hi = bins;                                      // keys[lo] == v; keys[hi] > v, or hi == bins
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (keys[mid] == v) lo = mid; else hi = mid;
        }
        const uint64_t cand = ((uint64_t)(hi - i) << 32) | (uint32_t)~v;
        best = cand > best ? cand : best;
    }
    best = wave_max_u64(best);
    ck::wave_sync();                                                     // the keys are read before the next pair writes them
    const uint32_t votes = (uint32_t)(best >> 32), key = ~(uint32_t)best;
    *aligned = votes >= P.min_votes;                                     // (min_votes >= 1: never without a vote)
    if (lane == 0) {
        if (*aligned) store_window(w, len_b, (uint32_t)b, key & 0x7FFFFFFFu, key >> 31);
        else store_window(w, len_b, (uint32_t)b, 0, 0);
        ck::store8((uint8_t*)(P.scores + 2 * pair), votes, matches);
    }
    return false;
}

// wave `wave` of `n_waves` takes pairs wave, wave + n_waves, ..
CK_DEV void pairs_wave(const Prealign& P, uint32_t* keys, uint64_t wave, uint64_t n_waves)
{
    uint64_t n_aligned = 0, n_invalid = 0;
    for (uint64_t p = wave; p < P.n_pairs; p += n_waves) {
        bool aligned;
        n_invalid += pair_wave(P, p, keys, &aligned);
        n_aligned += aligned;
    }
    if (ck::lane_id() == 0) {
        if (n_aligned) ck_sketch::global_add_u64(&P.totals[T_ALIGNED], n_aligned);
        if (n_invalid) ck_sketch::global_add_u64(&P.totals[T_INVALID], n_invalid);
    }
}

// ---- pairs of labels -----------------------------------------------------------------------------------------------------------
// lane `lane` of `n_lanes` takes records lane, lane + n_lanes, ..: pair i = (labels[i], i), a label of 2^32 or more as 0xFFFFFFFF
CK_DEV void labels_lane(const uint64_t* labels, uint64_t n_records, uint32_t* pairs, uint64_t lane, uint64_t n_lanes)
{
    for (uint64_t i = lane; i < n_records; i += n_lanes) {
        const uint64_t l = labels[i];
        ck::store8((uint8_t*)(pairs + 2 * i), l >> 32 ? NONE : (uint32_t)l, (uint32_t)i);
    }
}

}  // namespace ck_prealign
