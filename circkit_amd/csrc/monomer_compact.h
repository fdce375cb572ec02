// monomer_compact.h -- the writer closure of `circkit monomerize` for a device batch (the reference's src/monomerize.rs:94-131):
// decide() applies the writer's filters to one record's end index; gather_tile() packs the written monomers back to back.
// decide_uniq() is `circkit uniq`'s writer decision (src/uniq.rs:47-66) in the same form, for the same gather.
// Written against wave_prims.h only; every collective (ballot) sits in wave-uniform control flow, so the CPU fiber harness of
// tests/emu/ runs this source unchanged.
//
// The gather goes BY OUTPUT BYTES, not by records.  The output [out, out + B) is cut into granules of 16 bytes at 16-byte-
// aligned ABSOLUTE addresses (the caller's pointer needs no alignment: only the first and the last granule can be partial).
// A workgroup owns TILE_GRANULES consecutive granules, each of its GATHER_WAVES waves WAVE_GRANULES consecutive ones of
// them, and a wave covers its share in GATHER_STEPS steps of 64 granules: lane l of step s owns granule
// first + 64 * s + l, and nobody else ever touches that granule.
//  - the wave finds the output record that holds its first byte by a 64-way search in out_offsets (one probe per lane and
//    round: three rounds for 200 000 records);
//  - a lane then walks the records that overlap its granule, starting from where its previous granule ended (galloping in
//    out_offsets: with records of 1 kb nearly every granule lies inside one record and the walk is one comparison);
//  - each piece is ONE 16-byte load at the source address that puts the record's bytes where the granule wants them (lanes
//    of one record read contiguous memory), masked and OR-ed into the granule in registers;
//  - the finished granule is stored once: one aligned 16-byte store, or single bytes for a partial first / last granule.
// Every load stays inside the input payload [bytes + p0, bytes + p1): a window that would cross either end is loaded from
// the payload's first / last 16 bytes and shifted (monomerize.h's load16_safe does the same for a record's tail), and a
// payload of fewer than 16 bytes is read byte by byte.  Nothing is stored outside [out, out + B); the input is never written.
#pragma once
#include <stdint.h>
#include "wave_prims.h"

namespace ck_compact {

constexpr uint32_t NONE = 0xFFFFFFFFu;                  // = CIRCKIT_MONOMER_NONE
constexpr uint64_t WRITTEN = 1ull << 63;                // decide()'s result: this bit | the written length
constexpr uint32_t GATHER_WAVES = 4, GATHER_STEPS = 4;  // waves per workgroup; steps of 64 granules per wave and tile
constexpr uint32_t WAVE_GRANULES = 64 * GATHER_STEPS, TILE_GRANULES = WAVE_GRANULES * GATHER_WAVES;
constexpr uint32_t TILE_BYTES = 16 * TILE_GRANULES;     // 16 KiB of output per workgroup and tile

struct Filter {                                         // circkit_monomer_filter, validated by the host
    uint64_t min_length, max_length, min_overlap;
    double min_overlap_percent;
    uint32_t use_percent, keep_all;
};

// The writer's decision for one record of n symbols (src/monomerize.rs:94-131): full = full_seq().len(), e = the worker's end
// index.  Returns WRITTEN | the number of bytes written, or 0; *kept = the index that survives the filters, or NONE.
// An end beyond the record (nothing monomerize produces) counts as None before anything is derived from it.
CK_DEV uint64_t decide(uint64_t n, uint64_t full, uint32_t e, const Filter& F, uint32_t* kept)
{
    bool some = e != NONE && (uint64_t)e <= n;
    const uint64_t idx = e;
    if (some && (idx < F.min_length || idx > F.max_length)) some = false;
    const uint64_t over = full > idx ? full - idx : 0;  // callers owe full >= n >= idx
    if (some && over < F.min_overlap) some = false;
    if (some && F.use_percent) {
        // one IEEE f64 division (x / 0 is inf or NaN and never below the threshold; a NaN threshold never rejects)
        const double ratio = (double)over / (double)idx;
        if (ratio < F.min_overlap_percent) some = false;
    }
    *kept = some ? e : NONE;
    if (some) return WRITTEN | idx;
    return F.keep_all ? WRITTEN | n : 0;
}

// The same word for `circkit uniq` (src/uniq.rs:47-66: "emit the record, or write a table row"): record i of a batch whose
// record 0 has global index base is emitted, whole, iff it is the first with its hash: first_seen == base + i.  Any other
// value drops it, ~0 (the answer for a key that found no slot in the table) included.
CK_DEV uint64_t decide_uniq(uint64_t n, uint64_t first_seen, uint64_t base, uint64_t i)
{
    return first_seen == base + i ? WRITTEN | n : 0;
}

// ---- 64-way search, wave-uniform: the j in [0, m) with a[j] <= p < a[j + 1]; a[0] <= p < a[m] ----
CK_DEV uint64_t wave_find(const uint64_t* a, uint64_t m, uint64_t p)
{
    uint64_t lo = 0, hi = m;                            // a[lo] <= p < a[hi]
    const uint32_t lane = ck::lane_id();
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) / 64;      // < hi - lo
        const uint64_t at = lo + (uint64_t)(lane + 1) * step;
        const bool le = at < hi && a[at] <= p;          // true for a prefix of the lanes: a[] does not decrease
        const uint64_t cnt = (uint64_t)ck::popc64(ck::ballot(le));
        lo += cnt * step;
        if (lo + step < hi) hi = lo + step;
    }
    return lo;
}

// ---- the same for one lane that knows a[j] <= p: gallop upwards from j, then bisect ----
CK_DEV uint64_t lane_seek(const uint64_t* a, uint64_t m, uint64_t j, uint64_t p)
{
    if (a[j + 1] > p) return j;
    uint64_t lo = j + 1, step = 1, hi;                  // a[lo] <= p
    for (;;) {
        hi = m - lo > step ? lo + step : m;             // a[m] > p
        if (hi == m || a[hi] > p) break;
        lo = hi;
        step *= 2;
    }
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

struct u128 { uint64_t lo, hi; };

CK_DEV uint64_t low_bytes(uint32_t k) { return k >= 8 ? ~0ull : (1ull << (8 * k)) - 1ull; }     // k = 0..8
// bytes [b0, b1) of a granule, 0 <= b0 < b1 <= 16
CK_DEV u128 byte_range(uint32_t b0, uint32_t b1)
{
    u128 r;
    r.lo = low_bytes(b1 < 8 ? b1 : 8) & ~low_bytes(b0 < 8 ? b0 : 8);
    r.hi = low_bytes(b1 > 8 ? b1 - 8 : 0) & ~low_bytes(b0 > 8 ? b0 - 8 : 0);
    return r;
}
// byte k of the result = byte k + d of v (zero where that is outside), d = -15..15
CK_DEV u128 shift_bytes(u128 v, int d)
{
    u128 r = v;
    if (d > 0) {
        const uint32_t s = 8u * (uint32_t)d;
        if (s >= 64) { r.lo = s == 64 ? v.hi : v.hi >> (s - 64); r.hi = 0; }
        else { r.lo = (v.lo >> s) | (v.hi << (64 - s)); r.hi = v.hi >> s; }
    } else if (d < 0) {
        const uint32_t s = 8u * (uint32_t)(-d);
        if (s >= 64) { r.hi = s == 64 ? v.lo : v.lo << (s - 64); r.lo = 0; }
        else { r.hi = (v.hi << s) | (v.lo >> (64 - s)); r.lo = v.lo << s; }
    }
    return r;
}

// The 16 bytes at bytes[at .. at + 16), of which the caller uses only those inside the payload [p0, p1): no byte outside the
// payload is read.  at >= p0 - 15 and at < p1.
CK_DEV u128 load_window(const uint8_t* bytes, uint64_t p0, uint64_t p1, int64_t at)
{
    u128 r;
    if (at >= (int64_t)p0 && (uint64_t)at + 16 <= p1) {
        const ck::u32x4 v = ck::load16(bytes + at);
        r.lo = v.x | ((uint64_t)v.y << 32); r.hi = v.z | ((uint64_t)v.w << 32);
        return r;
    }
    if (p1 - p0 >= 16) {
        const int64_t from = at < (int64_t)p0 ? (int64_t)p0 : (int64_t)(p1 - 16);
        const ck::u32x4 v = ck::load16(bytes + from);
        r.lo = v.x | ((uint64_t)v.y << 32); r.hi = v.z | ((uint64_t)v.w << 32);
        return shift_bytes(r, (int)(at - from));
    }
    r.lo = r.hi = 0;
#pragma unroll 1
    for (uint32_t k = 0; k < 16; ++k) {                 // a payload of fewer than 16 bytes
        const int64_t pos = at + (int64_t)k;
        if (pos >= (int64_t)p0 && (uint64_t)pos < p1) {
            const uint64_t b = bytes[pos];
            if (k < 8) r.lo |= b << (8 * k); else r.hi |= b << (8 * (k - 8));
        }
    }
    return r;
}

struct Gather {
    const uint8_t* bytes;            // the input batch; its payload is bytes[p0 .. p1)
    uint64_t p0, p1;
    const uint64_t* out_offsets;     // m + 1 entries, out_offsets[0] = 0, out_offsets[m] = B
    const uint64_t* src_start;       // m entries: where in bytes[] output record j starts
    uint64_t m, B;
    uint8_t* out;
};

// One lane's granule: the output bytes [q, q + 16), q = its position relative to G.out (negative in a partial first granule).
// j: a record with out_offsets[j] <= max(q, 0); returns the record the granule's last byte lies in.
CK_DEV uint64_t gather_granule(const Gather& G, int64_t q, uint64_t j)
{
    uint64_t p = q < 0 ? 0 : (uint64_t)q;
    const uint64_t end = (uint64_t)(q + 16) < G.B ? (uint64_t)(q + 16) : G.B;
    u128 acc{ 0, 0 };
    while (p < end) {
        j = lane_seek(G.out_offsets, G.m, j, p);
        const uint64_t o = G.out_offsets[j], o1 = G.out_offsets[j + 1];
        const uint64_t e = o1 < end ? o1 : end;
        // the source byte of output position x is src_start[j] + (x - o): the window that starts at position q
        const int64_t at = (int64_t)G.src_start[j] + (q - (int64_t)o);
        const u128 v = load_window(G.bytes, G.p0, G.p1, at);
        const u128 mk = byte_range((uint32_t)((int64_t)p - q), (uint32_t)((int64_t)e - q));
        acc.lo |= v.lo & mk.lo;
        acc.hi |= v.hi & mk.hi;
        p = e;
    }
    if (q >= 0 && (uint64_t)q + 16 <= G.B) {
        ck::store16(G.out + q, ck::u32x4{ (uint32_t)acc.lo, (uint32_t)(acc.lo >> 32), (uint32_t)acc.hi, (uint32_t)(acc.hi >> 32) });
    } else {
#pragma unroll 1
        for (int64_t x = q < 0 ? 0 : q; x < (int64_t)end; ++x) {        // the first or the last granule of the whole output
            const uint32_t k = (uint32_t)(x - q);
            G.out[x] = (uint8_t)((k < 8 ? acc.lo >> (8 * k) : acc.hi >> (8 * (k - 8))) & 0xFF);
        }
    }
    return j;
}

// Tile `tile` of the output, run by every lane of a workgroup of GATHER_WAVES waves.  *first_record (when given) receives the
// record the wave's search found, for the harness to compare across lanes.
CK_DEV void gather_tile(const Gather& G, uint64_t tile, uint64_t* first_record = nullptr)
{
    if (G.B == 0) return;
    const uint64_t a0 = (uint64_t)(uintptr_t)G.out & 15u;                 // the output's position in its first granule
    const uint64_t n_gran = (a0 + G.B + 15) / 16;
    const uint64_t g0 = tile * TILE_GRANULES + (uint64_t)ck::wave_in_block() * WAVE_GRANULES;
    if (g0 >= n_gran) return;                                            // wave-uniform
    const int64_t q0 = (int64_t)(16 * g0) - (int64_t)a0;
    uint64_t j = wave_find(G.out_offsets, G.m, q0 < 0 ? 0 : (uint64_t)q0);
    if (first_record) *first_record = j;
    const uint32_t lane = ck::lane_id();
#pragma unroll 1
    for (uint32_t s = 0; s < GATHER_STEPS; ++s) {
        const uint64_t g = g0 + 64u * s + lane;
        if (g >= n_gran) break;
        j = gather_granule(G, (int64_t)(16 * g) - (int64_t)a0, j);
    }
}

}  // namespace ck_compact
