// monomerize.h -- the end of the first monomer of one record (the reference's lib/src/monomerize.rs:43-135:
// first_monomer_end_index, last_monomer_end_index, last_monomer_end_index_sensitive), computed by ONE WAVE per record.
// Written against wave_prims.h only; every collective (ballot / readlane / wave_sum) sits in wave-uniform control flow, so
// the CPU fiber harness of tests/emu/ runs this source unchanged.
//
// One pass on the prefix s[..m) (first_monomer_end_index): the seed is s[m-k..m); its occurrences p in s[..m-k) are visited
// in ascending order; for each, ovl = p + k and the pass ends with m - ovl when hamming(s[0..ovl), s[m-ovl..m)) <=
// max_dist(ovl).  Here:
//  - scan: a step tests BLOCK = 64 lanes x 16 positions.  A lane reads the 24 bytes behind its 16 positions with two 16-byte
//    loads (contiguous across the wave) and compares the first min(k, 8) seed bytes at each position in registers: a 16-bit
//    candidate mask per lane.  The candidates of the step are verified in ascending order (lowest lane, lowest bit first)
//    before the next step is looked at, so the first accepted one ends the pass (a poly-A record costs n/k short passes).
//  - verify: the last k bytes of the two overlap sides ARE the candidate and the seed (s[p..p+k) and s[m-k..m)), so the full
//    seed comparison is part of the mismatch count.  The count runs from the END of the overlap in steps of 1024 bytes (a
//    lane compares 16 bytes of each side); the first step also tells whether the k seed bytes are all equal (if not, p is no
//    occurrence), and the running count stops the candidate once it exceeds max_dist.
//  - last_monomer_end_index repeats the pass on the shrinking prefix.
// The sensitive form needs no reverse complement: bio's complement table is a bijection on bytes, so the pass on
// revcomp(s[..M)) is "the LARGEST q in [k, M-k] with s[q..q+k) == s[0..k) and hamming(s[0..M-q), s[q..M)) <= max_dist(M-q)":
// the same scan run downwards with the seed s[0..k), the same count run from the FRONT of the overlap.
//
// Every load stays inside [s, s + n): load16_safe() shifts the record's last 16 bytes for a window that crosses its end
// and assembles records of fewer than 16 bytes from single bytes (the only byte loads here).  n < 2^32.
#pragma once
#include <stdint.h>
#include "wave_prims.h"

namespace ck_mono {

constexpr uint32_t NONE = 0xFFFFFFFFu;         // = CIRCKIT_MONOMER_NONE
constexpr uint32_t BLOCK = 1024;               // positions per scan step, bytes per count step: 64 lanes x 16

struct Params {                                // validated by the host: 1 <= seed_len <= 63, 0 <= min_identity <= 1
    uint64_t overlap_dist;
    double min_identity;
    uint32_t seed_len, use_identity, sensitive;
};

// the 16 bytes at s[pos..pos+16), zero beyond the record
CK_DEV ck::u32x4 load16_safe(const uint8_t* s, uint64_t pos, uint32_t n)
{
    if (pos + 16 <= n) return ck::load16(s + pos);
    uint64_t lo = 0, hi = 0;
    if (pos < n) {
        if (n >= 16) {
            const ck::u32x4 v = ck::load16(s + (n - 16));
            const uint32_t sh = ((uint32_t)pos - (n - 16)) * 8u;                  // 8..120 bits
            const uint64_t vl = v.x | ((uint64_t)v.y << 32), vh = v.z | ((uint64_t)v.w << 32);
            if (sh >= 64) lo = vh >> (sh - 64);
            else { lo = (vl >> sh) | (vh << (64 - sh)); hi = vh >> sh; }
        } else {
#pragma unroll 1
            for (uint32_t j = 0; j < n - (uint32_t)pos; ++j) {                    // a record of fewer than 16 bytes
                const uint64_t b = s[(uint32_t)pos + j];
                if (j < 8) lo |= b << (8 * j); else hi |= b << (8 * (j - 8));
            }
        }
    }
    return ck::u32x4{ (uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32) };
}

// bit i = byte i of x is not zero
CK_DEV uint32_t nonzero_bytes4(uint32_t x)
{
    uint32_t m = ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u) >> 7;     // bits 0, 8, 16, 24
    m |= m >> 7;
    m |= m >> 14;
    return m & 0xFu;
}
// bit i = byte i of a differs from byte i of b
CK_DEV uint32_t differing_bytes16(const ck::u32x4& a, const ck::u32x4& b)
{
    return nonzero_bytes4(a.x ^ b.x) | (nonzero_bytes4(a.y ^ b.y) << 4) | (nonzero_bytes4(a.z ^ b.z) << 8) |
           (nonzero_bytes4(a.w ^ b.w) << 12);
}

// the first min(k, 8) bytes of a seed as two dwords with their masks
struct SeedHead { uint32_t lo, hi, mask_lo, mask_hi; };
CK_DEV SeedHead seed_head(const uint8_t* s, uint32_t at, uint32_t n, uint32_t k)
{
    const ck::u32x4 v = load16_safe(s, at, n);
    SeedHead h;
    h.mask_lo = k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u;
    h.mask_hi = k <= 4 ? 0u : k >= 8 ? 0xFFFFFFFFu : (1u << (8 * (k - 4))) - 1u;
    h.lo = v.x & h.mask_lo;
    h.hi = v.y & h.mask_hi;
    return h;
}

// a, b: the 32 bytes at a lane's first position (the last 8 unused).  Bit j = the seed head matches at position j.
CK_DEV uint32_t match16(const ck::u32x4& a, const ck::u32x4& b, const SeedHead& h)
{
    const uint32_t w[6] = { a.x, a.y, a.z, a.w, b.x, b.y };
    uint32_t hits = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int d = j >> 2, r = 8 * (j & 3);
        const uint32_t lo = r ? ck::alignbit(w[d + 1], w[d], (uint32_t)r) : w[d];
        const uint32_t hi = r ? ck::alignbit(w[d + 2], w[d + 1], (uint32_t)r) : w[d + 1];
        const uint32_t diff = ((lo ^ h.lo) & h.mask_lo) | ((hi ^ h.hi) & h.mask_hi);
        hits |= (diff == 0 ? 1u : 0u) << j;
    }
    return hits;
}

// lib/src/monomerize.rs:70-76.  One IEEE f64 multiply, floor, integer subtraction (nothing here can be contracted).
CK_DEV uint64_t max_dist(const Params& P, uint32_t ovl)
{
    if (!P.use_identity) return P.overlap_dist;
    const double prod = (double)ovl * P.min_identity;
    return (uint64_t)ovl - (uint64_t)__builtin_floor(prod);
}

// hamming(s[0..ovl), s[boff..boff+ovl)) <= md, and the k bytes of the seed zone (the last k of the overlap when FROM_END, the
// first k otherwise) all equal.  Wave-uniform result; ovl >= k >= 1, boff + ovl <= n.  Positions are 32-bit: every sum below
// stays under n.
template <bool FROM_END>
CK_DEV bool verify(const uint8_t* s, uint32_t n, uint32_t boff, uint32_t ovl, uint64_t md, uint32_t k)
{
    const uint32_t lane16 = 16u * ck::lane_id();
    uint64_t total = 0;
    for (uint32_t c = 0;; c += BLOCK) {
        const uint32_t rest = ovl - c;          // > 0
        uint32_t lo = 0, cnt = 0;               // this lane compares the overlap's bytes [lo, lo + cnt)
        if (lane16 < rest) {
            const uint32_t left = rest - lane16;
            cnt = left < 16 ? left : 16u;
            lo = FROM_END ? left - cnt : c + lane16;
        }
        uint32_t mm = 0;
        if (cnt) {
            const ck::u32x4 a = load16_safe(s, lo, n), b = load16_safe(s, (uint64_t)boff + lo, n);
            mm = differing_bytes16(a, b) & ((1u << cnt) - 1u);
        }
        if (c == 0) {
            uint32_t zone;
            if (FROM_END) {                     // positions >= ovl - k
                const uint32_t z0 = ovl - k;
                const uint32_t sh = z0 > lo ? z0 - lo : 0;
                zone = sh >= 16 ? 0u : mm >> sh;
            } else {                            // positions < k
                const uint32_t in = lo < k ? k - lo : 0;
                zone = in >= 16 ? mm : mm & ((1u << in) - 1u);
            }
            if (ck::ballot(zone != 0)) return false;
        }
        const uint32_t bad = (uint32_t)ck::popc32(mm);
        if (ck::ballot(bad != 0)) {
            total += ck::wave_sum_u64(bad);
            if (total > md) return false;
        }
        if (rest <= BLOCK) return true;
    }
}

// the 32 bytes behind the 16 positions of this lane that start at pos0
struct Window { ck::u32x4 a, b; };
CK_DEV Window load_window(const uint8_t* s, uint32_t pos0, uint32_t n)
{
    Window w;
    w.a = load16_safe(s, pos0, n);
    w.b = load16_safe(s, (uint64_t)pos0 + 16, n);
    return w;
}

// the candidates of a lane's 16 positions from pos0 on, of which only those up to pmax count
CK_DEV uint32_t window_hits(const Window& w, const SeedHead& h, uint32_t pos0, uint32_t pmax)
{
    uint32_t hits = match16(w.a, w.b, h);
    const uint32_t left = pmax - pos0;          // + 1 positions
    if (left < 15) hits &= (2u << left) - 1u;
    return hits;
}

// first_monomer_end_index on s[..m): the new end, or NONE
CK_DEV uint32_t pass_forward(const uint8_t* s, uint32_t n, uint32_t m, const Params& P)
{
    const uint32_t k = P.seed_len;
    if (m < 2 * k) return NONE;                 // m <= k: none; k < m < 2k: s[..m-k) is shorter than the seed
    const uint32_t pmax = m - 2 * k;            // the last position an occurrence may start at
    const SeedHead h = seed_head(s, m - k, n, k);
    const uint32_t lane16 = 16u * ck::lane_id();
    Window cur{}, nxt{};
    if (lane16 <= pmax) cur = load_window(s, lane16, n);
    for (uint32_t base = 0;; base += BLOCK) {
        const uint32_t rest = pmax - base;      // + 1 positions from base on
        if (rest >= BLOCK && lane16 <= rest - BLOCK) nxt = load_window(s, base + BLOCK + lane16, n);   // in flight meanwhile
        const uint32_t hits = lane16 <= rest ? window_hits(cur, h, base + lane16, pmax) : 0u;
        uint64_t lanes = ck::ballot(hits != 0);
        while (lanes) {
            const uint32_t l = (uint32_t)ck::ffs64(lanes);
            lanes &= lanes - 1;
            uint32_t hl = ck::readlane(hits, l);
            while (hl) {
                const uint32_t j = (uint32_t)ck::ffs32(hl);
                hl &= hl - 1;
                const uint32_t ovl = base + 16u * l + j + k;
                if (verify<true>(s, n, m - ovl, ovl, max_dist(P, ovl), k)) return m - ovl;
            }
        }
        if (rest < BLOCK) return NONE;
        cur = nxt;
    }
}

// first_monomer_end_index on revcomp(s[..M)), as an index into s: the largest q (see the head of this file), or NONE
CK_DEV uint32_t pass_backward(const uint8_t* s, uint32_t n, uint32_t M, const Params& P)
{
    const uint32_t k = P.seed_len;
    if (M < 2 * k) return NONE;
    const uint32_t pmin = k, pmax = M - k;
    const SeedHead h = seed_head(s, 0, n, k);
    const uint32_t lane16 = 16u * ck::lane_id();
    for (uint32_t base = pmax / (uint32_t)BLOCK * (uint32_t)BLOCK;; base -= BLOCK) {
        uint32_t hits = 0;
        if (lane16 <= pmax - base && (base + lane16 >= pmin || pmin - (base + lane16) < 16)) {
            const uint32_t pos0 = base + lane16;
            hits = window_hits(load_window(s, pos0, n), h, pos0, pmax);
            if (pos0 < pmin) hits &= ~((1u << (pmin - pos0)) - 1u);
        }
        uint64_t lanes = ck::ballot(hits != 0);
        while (lanes) {
            const uint32_t top = (uint32_t)(lanes >> 32);
            const uint32_t l = top ? 63u - (uint32_t)ck::clz32(top) : 31u - (uint32_t)ck::clz32((uint32_t)lanes);
            lanes &= ~(1ull << l);
            uint32_t hl = ck::readlane(hits, l);
            while (hl) {
                const uint32_t j = 31u - (uint32_t)ck::clz32(hl);
                hl &= ~(1u << j);
                const uint32_t q = base + 16u * l + j, ovl = M - q;
                if (verify<false>(s, n, q, ovl, max_dist(P, ovl), k)) return q;
            }
        }
        if (base <= pmin) return NONE;          // the steps below hold no position >= k
    }
}

// last_monomer_end_index[_sensitive] of the record s[0..n): the end index, or NONE.  Run by all 64 lanes of a wave with
// wave-uniform arguments; the result is wave-uniform.
CK_DEV uint32_t record_end(const uint8_t* s, uint32_t n, const Params& P)
{
    uint32_t res = NONE, m = n;
    for (;;) {
        const uint32_t r = pass_forward(s, n, m, P);
        if (r == NONE) break;
        res = r;
        m = r;
    }
    if (P.sensitive) {
        const uint32_t r = pass_backward(s, n, m, P);
        if (r != NONE) res = r;
    }
    return res;
}

}  // namespace ck_mono
