// window_gather.h -- cyclic windows of a device batch, packed back to back: window k writes `length` bytes read cyclically from
// position `start` of record `record`, on the record (strand 0) or on its reverse complement (strand 1).  One routine behind
// rotate (start = the rotation index, length n), cat (2n), decat (n / 2), revcomp (strand 1) and the ORF sequences of
// `circkit orfs` (Orf::seq_with_opts, lib/src/orfs.rs:19-35: start / length / strand as the ORF's).
// Written against wave_prims.h only; every collective (the ballot of wave_find) sits in wave-uniform control flow, so the CPU
// fiber harness of tests/emu/ runs this source unchanged.
//
// The gather goes BY OUTPUT BYTES, as monomer_compact.h's does and with its helpers: granules of 16 bytes at 16-byte-aligned
// ABSOLUTE addresses, one owner per granule, a 64-way search for the wave's first window, a galloping walk from window to
// window, one store per granule (single bytes in a partial first / last granule).  What is new is the source side.  Inside one
// window a granule consists of PIECES, each a maximal run that is contiguous in the source:
//  - a forward piece is the bytes u .. u + len of the record: ONE 16-byte load at the address that puts them where the granule
//    wants them, masked and OR-ed in;
//  - a reverse piece is the bytes n-1-u down to n-u-len: ONE 16-byte load at the mirrored address, the 16 bytes reversed in
//    registers and complemented through the 256-entry table `comp` (LDS on the device), then masked and OR-ed in;
//  - a piece ends where the record does (the window goes round: u returns to 0), so a granule over a record of fewer than 16
//    symbols is several pieces of that record: the same loop.
// Every load goes through ck_compact::load_window and stays inside the payload [bytes + p0, bytes + p1); nothing is stored
// outside [out, out + B); the input is never written.  Output positions, window lengths and B are 64-bit; a record's length,
// a start and a position inside a record are 32-bit (a window on a record of 2^32 symbols or more is invalid).
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "ck_scan.h"
#include "monomer_compact.h"

namespace ck_windows {

using ck_compact::u128;

struct Window {                                          // = circkit_window
    uint64_t length;
    uint32_t record, start, strand, reserved;
};

constexpr uint32_t GATHER_WAVES = 4, GATHER_STEPS = 4;   // waves per workgroup; steps of 64 granules per wave and tile
constexpr uint32_t WAVE_GRANULES = 64 * GATHER_STEPS, TILE_GRANULES = WAVE_GRANULES * GATHER_WAVES;
constexpr uint32_t TILE_BYTES = 16 * TILE_GRANULES;      // 16 KiB of output per workgroup and tile

// The bytes window W writes: its length, or 0 on an empty record (cycle() over an empty slice yields nothing) and for an
// invalid window, which sets *invalid and is never dereferenced: a record beyond the batch, a strand other than 0 / 1, a
// reserved word in use, a record of 2^32 symbols or more.
CK_DEV uint64_t effective_length(const Window& W, const uint64_t* offsets, uint64_t n_records, bool* invalid)
{
    *invalid = true;
    if ((uint64_t)W.record >= n_records || W.strand > 1 || W.reserved != 0) return 0;
    const uint64_t n = offsets[(uint64_t)W.record + 1] - offsets[W.record];
    if (n > 0xFFFFFFFFull) return 0;
    *invalid = false;
    return n ? W.length : 0;
}

// a + b, or ~0 where that does not fit: the scan of the lengths stays monotone whatever lengths the windows name, and a batch
// whose total does not fit 64 bits has the total ~0, which no capacity holds
using ck_scan::sat_add;

// (a + t) mod n for a < n: the one 64-bit division of a (granule, window) pair, and none where the window has not yet gone
// round its record twice
CK_DEV uint32_t cyc_add(uint32_t a, uint64_t t, uint32_t n)
{
    uint64_t u = (uint64_t)a + t;                        // a < 2^32: wraps only for t >= 2^64 - 2^32
    if (u < t) u = (uint64_t)a + t % n;
    if (u < n) return (uint32_t)u;
    if (u < 2ull * n) return (uint32_t)(u - n);
    return (uint32_t)(u % n);
}

// the 16 bytes of v in reverse order, each through the table
CK_DEV u128 reverse_complement16(u128 v, const uint8_t* comp)
{
    const uint64_t a = __builtin_bswap64(v.hi), b = __builtin_bswap64(v.lo);
    u128 r{ 0, 0 };
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        r.lo |= (uint64_t)comp[(a >> (8 * k)) & 0xFF] << (8 * k);
        r.hi |= (uint64_t)comp[(b >> (8 * k)) & 0xFF] << (8 * k);
    }
    return r;
}

struct Gather {
    const uint8_t* bytes;            // the input batch; its payload is bytes[p0 .. p1)
    const uint64_t* offsets;         // n_records + 1 entries
    uint64_t p0, p1;
    const Window* windows;           // m entries; a window with out_offsets[k] == out_offsets[k + 1] is never read
    const uint64_t* out_offsets;     // m + 1 entries, out_offsets[0] = 0, out_offsets[m] = B
    uint64_t m, B;
    const uint8_t* comp;             // 256 entries
    uint8_t* out;
};

// One lane's granule: the output bytes [q, q + 16), q = its position relative to G.out (negative in a partial first granule).
// j: a window with out_offsets[j] <= max(q, 0); returns the window the granule's last byte lies in.
CK_DEV uint64_t gather_granule(const Gather& G, int64_t q, uint64_t j)
{
    uint64_t p = q < 0 ? 0 : (uint64_t)q;
    const uint64_t end = (uint64_t)(q + 16) < G.B ? (uint64_t)(q + 16) : G.B;
    u128 acc{ 0, 0 };
    while (p < end) {
        j = ck_compact::lane_seek(G.out_offsets, G.m, j, p);
        const uint64_t o = G.out_offsets[j], o1 = G.out_offsets[j + 1];          // o <= p < o1: the window is valid, its record not empty
        const uint64_t e = o1 < end ? o1 : end;
        const Window W = G.windows[j];
        const uint64_t r0 = G.offsets[W.record];
        const uint32_t n = (uint32_t)(G.offsets[(uint64_t)W.record + 1] - r0);
        uint32_t u = cyc_add(W.start < n ? W.start : W.start % n, p - o, n);     // output byte p is symbol u of the strand
        while (p < e) {                                                          // one piece: symbols u .. u + len, no wrap inside
            const uint64_t room = (uint64_t)(n - u), want = e - p;
            const uint32_t len = (uint32_t)(want < room ? want : room);          // 1 .. 16
            const uint32_t b0 = (uint32_t)((int64_t)p - q);                      // the piece's first byte in the granule
            u128 v;
            if (W.strand == 0) {
                // granule byte b0 + i = record byte u + i: the 16 bytes that start b0 in front of record byte u
                v = ck_compact::load_window(G.bytes, G.p0, G.p1, (int64_t)(r0 + u) - (int64_t)b0);
            } else {
                // granule byte b0 + i = comp(record byte n-1-u - i): reversed, granule byte k is loaded byte 15 - k, so the load
                // starts 15 - b0 in front of record byte n-1-u
                v = ck_compact::load_window(G.bytes, G.p0, G.p1, (int64_t)(r0 + (n - 1 - u)) - (int64_t)(15 - b0));
                v = reverse_complement16(v, G.comp);
            }
            const u128 mk = ck_compact::byte_range(b0, b0 + len);
            acc.lo |= v.lo & mk.lo;
            acc.hi |= v.hi & mk.hi;
            p += len;
            u += len;
            if (u == n) u = 0;
        }
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

// Tile `tile` of the output, run by every lane of a workgroup of GATHER_WAVES waves.  *first_window (when given) receives the
// window the wave's search found, for the harness to compare across lanes.
CK_DEV void gather_tile(const Gather& G, uint64_t tile, uint64_t* first_window = nullptr)
{
    if (G.B == 0) return;
    const uint64_t a0 = (uint64_t)(uintptr_t)G.out & 15u;                 // the output's position in its first granule
    const uint64_t n_gran = (a0 + G.B + 15) / 16;
    const uint64_t g0 = tile * TILE_GRANULES + (uint64_t)ck::wave_in_block() * WAVE_GRANULES;
    if (g0 >= n_gran) return;                                            // wave-uniform
    const int64_t q0 = (int64_t)(16 * g0) - (int64_t)a0;
    uint64_t j = ck_compact::wave_find(G.out_offsets, G.m, q0 < 0 ? 0 : (uint64_t)q0);
    if (first_window) *first_window = j;
    const uint32_t lane = ck::lane_id();
#pragma unroll 1
    for (uint32_t s = 0; s < GATHER_STEPS; ++s) {
        const uint64_t g = g0 + 64u * s + lane;
        if (g >= n_gran) break;
        j = gather_granule(G, (int64_t)(16 * g) - (int64_t)a0, j);
    }
}

// ---- one window per record (rotate / cat / decat / revcomp: src/rotate.rs:26-40, src/concatenate.rs:21-22,45) ----
enum { KIND_ROTATE_BASES, KIND_ROTATE_PERCENT, KIND_CAT, KIND_DECAT, KIND_REVCOMP, N_KINDS };

// floor(n as f64 * percent) as i64, as Rust's `as` converts: NaN is 0, anything beyond the range is the range's end
CK_DEV int64_t percent_shift(uint64_t n, double percent)
{
    const double v = __builtin_floor((double)n * percent);
    if (v != v) return 0;
    if (v >= 9223372036854775808.0) return INT64_MAX;
    if (v <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)v;
}

CK_DEV Window window_of_record(uint64_t n, uint32_t record, uint32_t kind, int64_t bases, double percent)
{
    Window W{ n, record, 0, 0, 0 };
    if (kind == KIND_CAT) W.length = sat_add(n, n);
    else if (kind == KIND_DECAT) W.length = n / 2;
    else if (kind == KIND_REVCOMP) W.strand = 1;
    else if (n != 0 && n <= 0xFFFFFFFFull) {             // (a longer record's window is invalid whatever its start)
        const int64_t s = kind == KIND_ROTATE_PERCENT ? percent_shift(n, percent) : bases;
        const uint64_t mag = s >= 0 ? (uint64_t)s : 0ull - (uint64_t)s;          // |i64::MIN| = 2^63
        const uint64_t idx = s >= 0 ? n - mag % n : mag % n;
        W.start = (uint32_t)(idx % n);
    }
    if (n == 0) W.length = 0;
    return W;
}

}  // namespace ck_windows
