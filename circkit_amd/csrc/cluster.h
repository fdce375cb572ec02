// cluster.h -- candidate pairs from the sketch rows (LSH banding) and single linkage over scored pairs: the "clusters of circular
// records" section of include/circkit.h, which is the definition.  Written against wave_prims.h only (and sketch.h for fmix64 and
// EMPTY: one hash, one empty bin); every collective (ballot, readlane, wave_sum_u64) sits in wave-uniform control flow, so the CPU
// fiber harness of tests/emu/ runs this source unchanged.
//
// Candidates, four steps of which the second is the uniq unit's:
//   keys_lane    one lane per (record, band): band_bins 8-byte loads and as many fmix64 -> keys[i * n_bands + b], NO_KEY where a
//                bin of the band is EMPTY (or the key itself came out as ~0)
//   (resolve)    first_pos[p] = the smallest position with an equal key; rep = first_pos / n_bands, the smallest record with that key
//   count_wave   one wave per record, lane = band: the bands that propose a pair (rep < i, and no earlier band of the record
//                proposed the same rep) as a 64-bit mask per record, and their number
//   write_wave   after the scan of the numbers: the pairs (rep, i) at the record's offset in band order, when all of them lie
//                below the capacity
// Link, three steps over a parent array of 32-bit indices:
//   init_lane    parent[i] = i
//   link_lane    one lane per pair: the threshold, then a lock-free union by compare-and-swap (see unite)
//   flatten_lane labels[i] = the root of i, and the number of roots; parent is only read
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "sketch.h"

namespace ck_cluster {

constexpr uint64_t NO_KEY = ~0ull;
constexpr uint64_t GOLDEN = 0x9e3779b97f4a7c15ull;
constexpr uint32_t N_BANDS_MAX = 64, BAND_BINS_MAX = 16;
constexpr uint32_t SCAN_WG = 256, SCAN_ITEMS = 2, SCAN_TILE = SCAN_WG * SCAN_ITEMS;      // of the scan of the records' pair counts
enum { C_TOTAL, C_OVERFLOW, C_WORDS };                   // the totals of a candidates call, in device memory: the pairs; the keys
                                                         // of its own resolve that found no slot (the low 32 bits)
enum { L_CLUSTERS, L_LINKED, L_INVALID, L_WORDS };       // the totals of a link

// The 32-bit accesses to the parent array while other workgroups change it.  A read goes past this CU's L1 (an agent-scope
// relaxed load), the two writes are agent-scope atomics.  The fibers of the CPU harness do not preempt each other between
// collectives, so plain accesses are the same there.
#ifdef CK_WAVE_PRIMS_OVERRIDE
CK_DEV uint32_t parent_load(const uint32_t* p) { return *p; }
CK_DEV uint32_t parent_cas(uint32_t* p, uint32_t expected, uint32_t v) { const uint32_t o = *p; if (o == expected) *p = v; return o; }
CK_DEV void parent_min(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
#else
CK_DEV uint32_t parent_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
CK_DEV uint32_t parent_cas(uint32_t* p, uint32_t expected, uint32_t v) { return atomicCAS(p, expected, v); }
CK_DEV void parent_min(uint32_t* p, uint32_t v) { atomicMin(p, v); }
#endif

// ---- band keys -----------------------------------------------------------------------------------------------------------------
struct Keys {
    const uint64_t* rows;            // n_records << log2_bins
    uint64_t n_records;
    uint32_t log2_bins, n_bands, band_bins;
    uint64_t* keys;                  // n_records * n_bands
};

// the key of band b over band[0 .. band_bins)
CK_DEV uint64_t band_key(const uint64_t* band, uint32_t b, uint32_t band_bins)
{
    uint64_t x = (uint64_t)(b + 1) * GOLDEN;
    bool empty = false;
    for (uint32_t j = 0; j < band_bins; ++j) {
        const uint64_t v = band[j];
        empty |= v == ck_sketch::EMPTY;
        x = ck_sketch::fmix64(x ^ v);
    }
    return empty ? NO_KEY : x;
}

// lane `lane` of `n_lanes` takes the positions lane, lane + n_lanes, ..  (n_records * n_bands < 2^32 - 1: the ABI checks)
CK_DEV void keys_lane(const Keys& K, uint64_t lane, uint64_t n_lanes)
{
    const uint64_t total = K.n_records * K.n_bands;
    for (uint64_t at = lane; at < total; at += n_lanes) {
        const uint32_t i = (uint32_t)at / K.n_bands, b = (uint32_t)at - i * K.n_bands;
        K.keys[at] = band_key(K.rows + ((uint64_t)i << K.log2_bins) + (uint64_t)b * K.band_bins, b, K.band_bins);
    }
}

// ---- candidate pairs -----------------------------------------------------------------------------------------------------------
struct Emit {
    const uint64_t* keys;            // n_records * n_bands
    const uint64_t* first_pos;       // n_records * n_bands: the smallest position with an equal key (~0: the key found no slot)
    uint64_t n_records;
    uint32_t n_bands;
    uint64_t* masks;                 // n_records: bit b = band b of the record proposes a pair
    uint64_t* offsets;               // n_records + 1: count_wave writes the numbers to [1 ..], the scan makes them the ends
    uint32_t* pairs;                 // 2 * capacity
    uint64_t capacity;
};

// One record by one wave, lane = band: the mask of the bands that propose a pair (wave-uniform).
CK_DEV uint64_t proposing_bands(const Emit& E, uint64_t rec)
{
    const uint32_t lane = ck::lane_id();
    const bool in = lane < E.n_bands;
    const uint64_t at = rec * E.n_bands + lane;
    const uint64_t key = in ? E.keys[at] : NO_KEY, fp = in ? E.first_pos[at] : ~0ull;
    const uint32_t rep = (uint32_t)fp / E.n_bands;                       // (fp < 2^32 - 1 or ~0, which `valid` rules out)
    const bool valid = in && key != NO_KEY && fp != ~0ull && rep < rec;
    const uint64_t vmask = ck::ballot(valid);
    bool dup = false;
    for (uint32_t b = 0; b + 1 < E.n_bands; ++b) {                       // the first band wins: at most 63 broadcasts
        const uint32_t r = ck::readlane(rep, b);
        dup |= ((vmask >> b) & 1) != 0 && lane > b && r == rep;
    }
    return ck::ballot(valid && !dup);
}

// wave `wave` of `n_waves` takes records wave, wave + n_waves, ..
CK_DEV void count_wave(const Emit& E, uint64_t wave, uint64_t n_waves)
{
    for (uint64_t rec = wave; rec < E.n_records; rec += n_waves) {
        const uint64_t mask = proposing_bands(E, rec);
        if (ck::lane_id() == 0) {
            E.masks[rec] = mask;
            E.offsets[rec + 1] = (uint64_t)ck::popc64(mask);
        }
    }
}

// behind the scan: a record all of whose pairs lie below the capacity is written, (rep, record) per proposing band in band order
CK_DEV void write_wave(const Emit& E, uint64_t wave, uint64_t n_waves)
{
    const uint32_t lane = ck::lane_id();
    for (uint64_t rec = wave; rec < E.n_records; rec += n_waves) {
        const uint64_t mask = E.masks[rec], start = E.offsets[rec], end = E.offsets[rec + 1];
        if (end > E.capacity || ((mask >> lane) & 1) == 0) continue;
        const uint64_t p = start + (uint64_t)ck::popc64(mask & ((1ull << lane) - 1));
        const uint32_t rep = (uint32_t)E.first_pos[rec * E.n_bands + lane] / E.n_bands;
        ck::store8((uint8_t*)(E.pairs + 2 * p), rep, (uint32_t)rec);
    }
}

// ---- link ----------------------------------------------------------------------------------------------------------------------
struct Link {
    uint64_t n_records;
    const uint32_t* pairs;           // (i, j) * n_pairs
    const uint32_t* scores;          // (match, filled) * n_pairs
    uint64_t n_pairs;
    uint32_t min_similarity_q16, min_filled;
    uint32_t* parent;                // n_records
    uint64_t* labels;                // n_records
    uint64_t* totals;                // L_WORDS
};

CK_DEV void init_lane(const Link& L, uint64_t lane, uint64_t n_lanes)
{
    for (uint64_t i = lane; i < L.n_records; i += n_lanes) L.parent[i] = (uint32_t)i;
}

// The root of x as far as this lane can see it: every value read was parent[.] at some instant, so the walk descends through
// (former) ancestors of x and ends.  Path halving on the way: parent[x] becomes min(parent[x], its grandparent as read), which
// keeps parent[x] <= x, keeps x in its tree and never touches a root (p != x was read, and a record that has a parent keeps one).
CK_DEV uint32_t find_root(uint32_t* parent, uint32_t x, bool halve)
{
    for (;;) {
        const uint32_t p = parent_load(parent + x);
        if (p == x) return x;
        const uint32_t g = parent_load(parent + p);
        if (halve && g != p) parent_min(parent + x, g);
        x = g;
    }
}

CK_DEV void unite(uint32_t* parent, uint32_t i, uint32_t j)
{
    uint32_t a = find_root(parent, i, true), b = find_root(parent, j, true);
    while (a != b) {
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        // INVARIANT: parent[x] <= x for every x at every instant.  The only writes are this one (lo < hi, and only where
        // parent[hi] == hi still holds, so a root alone ever gets a parent) and the halving above (a smaller former ancestor).
        // So no chain of parents can cycle, every root is the minimum of its tree, and every walk ends.  A failed swap returns
        // the parent hi has got meanwhile, which is < hi: the retry starts from there, below where it was, whatever a stale
        // read said before.
        const uint32_t seen = parent_cas(parent + hi, hi, lo);
        if (seen == hi) return;
        a = find_root(parent, seen, true);
        b = lo;
    }
}

// lane `lane` of `n_lanes` takes pairs lane, lane + n_lanes, ..; every lane of a wave comes here (the sums are the wave's)
CK_DEV void link_lane(const Link& L, uint64_t lane, uint64_t n_lanes)
{
    uint64_t linked = 0, invalid = 0;
    for (uint64_t p = lane; p < L.n_pairs; p += n_lanes) {
        const uint32_t i = L.pairs[2 * p], j = L.pairs[2 * p + 1];
        if (i >= L.n_records || j >= L.n_records) { ++invalid; continue; }
        if (i == j) continue;
        const uint32_t match = L.scores[2 * p], filled = L.scores[2 * p + 1];
        if (filled < L.min_filled || ((uint64_t)match << 16) < (uint64_t)L.min_similarity_q16 * filled) continue;
        ++linked;
        unite(L.parent, i, j);
    }
    linked = ck::wave_sum_u64(linked);
    invalid = ck::wave_sum_u64(invalid);
    if (ck::lane_id() == 0) {
        if (linked) ck_sketch::global_add_u64(&L.totals[L_LINKED], linked);
        if (invalid) ck_sketch::global_add_u64(&L.totals[L_INVALID], invalid);
    }
}

// behind the link (another launch: nothing changes parent any more)
CK_DEV void flatten_lane(const Link& L, uint64_t lane, uint64_t n_lanes)
{
    uint64_t roots = 0;
    for (uint64_t i = lane; i < L.n_records; i += n_lanes) {
        const uint32_t r = find_root(L.parent, (uint32_t)i, false);
        L.labels[i] = r;
        roots += r == i;
    }
    roots = ck::wave_sum_u64(roots);
    if (roots && ck::lane_id() == 0) ck_sketch::global_add_u64(&L.totals[L_CLUSTERS], roots);
}

}  // namespace ck_cluster
