// distance.h -- the bounded edit distance of two records: the "edit distance of record pairs" section of include/circkit.h, which
// is the definition.  One pair by one wave, by furthest-reaching diagonals (Landau-Vishkin / Ukkonen): round e holds, for every
// diagonal k = j - i in -e .. e, the furthest row i of x that e edits reach; the distance is the first e at which the diagonal
// n_y - n_x reaches row n_x.  The cost is O(n + W^2), not O(n W): most of a pair's work is one long run of equal bytes.  Written
// against wave_prims.h only (and sketch.h for TOO_LONG and the 64-bit add); every collective (ballot, readlane, uniform,
// wave_sync) sits in wave-uniform control flow, so the CPU fiber harness of tests/emu/ runs this source unchanged.
//
//   The wave's slice of LDS (SLICE_WORDS words): two rows of row_words(W) words, then the stage.  Both records are copied into the
//   stage when n_x + n_y + STAGE_SLACK <= stage_bytes(W), each at a multiple of 16 bytes, so that every word load is aligned and the
//   8 bytes at any position are two alignbits of three words.  Records that do not fit are read from global memory through the same
//   accessor (get8), which there never touches a byte outside the record.
//   Round 0 is the whole wave's: 64 lanes x 8 bytes a step on the main diagonal, the first lane that stops found by a ballot.
//   Rounds 1 .. W: a lane takes diagonals lane, lane + 64, ..; the three neighbours of the previous round are plain LDS reads.
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "sketch.h"

namespace ck_distance {

constexpr uint32_t OVER = 0xFFFFFFFFu;                   // CIRCKIT_DISTANCE_OVER
constexpr uint32_t DISTANCE_MAX = 255;                   // CIRCKIT_DISTANCE_MAX
constexpr uint32_t DISTANCE_WAVES = 4;                   // waves per workgroup, each with SLICE_WORDS words of LDS
constexpr uint32_t SLICE_WORDS = 1280;                   // 5 KiB a wave: 32 waves a CU in 160 KiB, what 64 VGPRs allow
constexpr uint32_t STAGE_SLACK = 48;                     // two roundings to 16 bytes, and the two words an 8-byte read may run over
constexpr int32_t NEG = -0x40000000;                     // a diagonal that no path has reached
enum { T_WITHIN, T_INVALID, T_WORDS };                   // the totals of a pairs call, in device memory

// words of one row: diagonals -W .. W and a NEG on either side, rounded so that the stage starts at a multiple of 16 bytes
CK_DEV uint32_t row_words(uint32_t W) { return (2 * W + 3 + 3) & ~3u; }
CK_DEV uint32_t stage_bytes(uint32_t W) { return 4 * (SLICE_WORDS - 2 * row_words(W)); }

struct Distance {
    const uint8_t* bytes_a;          // batch A
    const uint64_t* offsets_a;       // n_a + 1
    uint64_t n_a;
    const uint8_t* bytes_b;          // batch B (may be A)
    const uint64_t* offsets_b;       // n_b + 1
    uint64_t n_b;
    uint32_t max_distance;           // W
    const uint32_t* pairs;           // (i, j) * n_pairs
    uint64_t n_pairs;
    uint32_t* distance;              // n_pairs, or null
    uint32_t* scores;                // (L - d, L) * n_pairs, or null
    uint64_t* totals;                // T_WORDS
};

struct Rec {
    const uint8_t* g;                // the record in global memory
    const uint32_t* lds;             // its copy in the stage (STAGED only)
    uint32_t n;
};

// The record's bytes pos .. pos + 7 (pos < n), the first in the low byte of lo.  Bytes at n and beyond are arbitrary: the caller
// counts at most n - pos of them.  From global memory nothing outside the record is read.
template <bool STAGED>
CK_DEV void get8(const Rec& r, uint32_t pos, uint32_t& lo, uint32_t& hi)
{
    if (STAGED) {
        const uint32_t* w = r.lds + (pos >> 2);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], sh = (pos & 3u) * 8u;
        lo = ck::alignbit(w1, w0, sh);
        hi = ck::alignbit(w2, w1, sh);
    } else {
        const uint8_t* p = r.g + pos;
        const uint32_t left = r.n - pos;
        if (left >= 8) {
            lo = ck::load4(p);
            hi = ck::load4(p + 4);
        } else {
            uint64_t v = 0;
            for (uint32_t b = 0; b < left; ++b) v |= (uint64_t)p[b] << (8 * b);
            lo = (uint32_t)v;
            hi = (uint32_t)(v >> 32);
        }
    }
}

// the number of leading equal bytes of two 8-byte groups
CK_DEV uint32_t match8(uint32_t alo, uint32_t ahi, uint32_t blo, uint32_t bhi)
{
    const uint32_t dl = alo ^ blo, dh = ahi ^ bhi;
    return dl ? (uint32_t)ck::ffs32(dl) >> 3 : dh ? 4u + ((uint32_t)ck::ffs32(dh) >> 3) : 8u;
}

// x[i ..) against y[j ..): the leading equal bytes of the next 8, at most `room` (room >= 1); 8 means the run goes on
template <bool STAGED>
CK_DEV uint32_t step8(const Rec& X, uint32_t i, const Rec& Y, uint32_t j, uint32_t room)
{
    uint32_t alo, ahi, blo, bhi;
    get8<STAGED>(X, i, alo, ahi);
    get8<STAGED>(Y, j, blo, bhi);
    const uint32_t m = match8(alo, ahi, blo, bhi);
    return m < room ? m : room;
}

// the record into the stage: 16 bytes a lane where they are whole, the last ones byte by byte (lds at a multiple of 16 bytes)
CK_DEV void stage(const uint8_t* g, uint32_t n, uint32_t* lds)
{
    for (uint32_t c = 16 * ck::lane_id(); c < n; c += 1024) {
        if (n - c >= 16) {
            ck::lds_store16(lds + (c >> 2), ck::load16(g + c));
        } else {
            for (uint32_t w = 0; 4 * w < n - c; ++w) {
                uint32_t v = 0;
                for (uint32_t b = 0; b < 4 && c + 4 * w + b < n; ++b) v |= (uint32_t)g[c + 4 * w + b] << (8 * b);
                lds[(c >> 2) + w] = v;
            }
        }
    }
}

// lev(x, y) if it is at most W, OVER otherwise (wave-uniform).  |n_x - n_y| <= W; n_x, n_y < 2^31.
template <bool STAGED>
CK_DEV uint32_t lev_wave(const uint8_t* gx, uint32_t n_x, const uint8_t* gy, uint32_t n_y, uint32_t W, uint32_t* slice)
{
    const uint32_t lane = ck::lane_id(), rw = row_words(W);
    int32_t *prev = (int32_t*)slice, *cur = prev + rw;
    uint32_t* st = slice + 2 * rw;
    const Rec X{ gx, st, n_x }, Y{ gy, st + (((n_x + 15u) >> 4) << 2), n_y };
    ck::wave_sync();                                                     // the pair before has read its slice
    if (STAGED) {
        stage(gx, n_x, st);
        stage(gy, n_y, st + (((n_x + 15u) >> 4) << 2));
    }
    for (uint32_t t = lane; t < 2 * rw; t += 64) prev[t] = NEG;          // both rows
    ck::wave_sync();
    // round 0, the whole wave on the main diagonal: 512 bytes a step
    const uint32_t n_min = n_x < n_y ? n_x : n_y;
    uint32_t reach;
    for (uint32_t base = 0;; base += 512) {
        const uint32_t pos = base + 8 * lane;
        uint32_t m = 0;
        if (pos < n_min) m = step8<STAGED>(X, pos, Y, pos, n_min - pos);
        const uint64_t stopped = ck::ballot(m < 8);                      // a lane at or past n_min has m = 0: the loop ends
        if (stopped) {
            const uint32_t first = (uint32_t)ck::ffs64(stopped);
            reach = base + 8 * first + ck::readlane(m, first);
            break;
        }
    }
    const int32_t kd = (int32_t)n_y - (int32_t)n_x, mid = (int32_t)W + 1;      // diagonal k lies at word k + mid
    if (kd == 0 && reach == n_x) return 0;
    if (lane == 0) prev[mid] = (int32_t)reach;
    ck::wave_sync();
    for (uint32_t e = 1; e <= W; ++e) {
        // the diagonals of the matrix among -e .. e; each has a neighbour that round e - 1 reached
        const int32_t klo = e < n_x ? -(int32_t)e : -(int32_t)n_x, khi = e < n_y ? (int32_t)e : (int32_t)n_y;
        bool found = false;
        for (int32_t k = klo + (int32_t)lane; k <= khi; k += 64) {
            const int32_t sub = prev[mid + k] + 1, ins = prev[mid + k - 1], del = prev[mid + k + 1] + 1;
            int32_t t = sub > ins ? sub : ins;
            t = del > t ? del : t;
            const int32_t room_y = (int32_t)n_y - k, last = (int32_t)n_x < room_y ? (int32_t)n_x : room_y;      // the diagonal's last row
            t = t < last ? t : last;
            if (t < 0) { cur[mid + k] = NEG; continue; }                 // (never: see above)
            uint32_t i = (uint32_t)t;
            while (i < (uint32_t)last) {
                const uint32_t m = step8<STAGED>(X, i, Y, (uint32_t)((int32_t)i + k), (uint32_t)last - i);
                i += m;
                if (m < 8) break;
            }
            cur[mid + k] = (int32_t)i;
            found = found || (k == kd && i == n_x);
        }
        ck::wave_sync();
        if (ck::ballot(found)) return e;
        int32_t* s = prev; prev = cur; cur = s;
    }
    return OVER;
}

// One pair by one wave.  *within: whether the distance is at most W.  Returns whether the pair is invalid (both wave-uniform).
CK_DEV bool pair_wave(const Distance& D, uint64_t pair, uint32_t* slice, bool* within)
{
    const uint64_t i = ck::uniform(D.pairs[2 * pair]), j = ck::uniform(D.pairs[2 * pair + 1]);      // (scalars: every branch below is the wave's)
    const uint32_t W = D.max_distance;
    *within = false;
    bool invalid = i >= D.n_a || j >= D.n_b;
    uint64_t x0 = 0, y0 = 0, len_x = 0, len_y = 0;
    if (!invalid) {
        x0 = ck::uniform64(D.offsets_a[i]); len_x = ck::uniform64(D.offsets_a[i + 1]) - x0;
        y0 = ck::uniform64(D.offsets_b[j]); len_y = ck::uniform64(D.offsets_b[j + 1]) - y0;
        invalid = len_x >= ck_sketch::TOO_LONG || len_y >= ck_sketch::TOO_LONG;
    }
    uint32_t d = OVER, L = 0;
    if (!invalid) {
        const uint32_t n_x = (uint32_t)len_x, n_y = (uint32_t)len_y;
        L = n_x > n_y ? n_x : n_y;
        if (L - (n_x < n_y ? n_x : n_y) <= W) {                          // the length gate: no byte is read before it
            if (len_x + len_y + STAGE_SLACK <= stage_bytes(W)) d = lev_wave<true>(D.bytes_a + x0, n_x, D.bytes_b + y0, n_y, W, slice);
            else d = lev_wave<false>(D.bytes_a + x0, n_x, D.bytes_b + y0, n_y, W, slice);
        }
        *within = d != OVER;
    }
    if (ck::lane_id() == 0) {
        if (D.distance) ck::store4((uint8_t*)(D.distance + pair), d);
        if (D.scores) ck::store8((uint8_t*)(D.scores + 2 * pair), d != OVER ? L - d : 0u, L);
    }
    return invalid;
}

// wave `wave` of `n_waves` takes pairs wave, wave + n_waves, ..
CK_DEV void pairs_wave(const Distance& D, uint32_t* slice, uint64_t wave, uint64_t n_waves)
{
    uint64_t n_within = 0, n_invalid = 0;
    for (uint64_t p = wave; p < D.n_pairs; p += n_waves) {
        bool within;
        n_invalid += pair_wave(D, p, slice, &within);
        n_within += within;
    }
    if (ck::lane_id() == 0) {
        if (n_within) ck_sketch::global_add_u64(&D.totals[T_WITHIN], n_within);
        if (n_invalid) ck_sketch::global_add_u64(&D.totals[T_INVALID], n_invalid);
    }
}

}  // namespace ck_distance
