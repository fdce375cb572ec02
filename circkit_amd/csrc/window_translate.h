// window_translate.h -- the proteins of cyclic windows of a device batch, packed back to back: window k writes length / 3
// residues, residue t the translation of the three symbols (start + 3t .. start + 3t + 2) mod n of the strand window_gather.h
// defines, through a 64-entry table in the order of NCBI's genetic-code strings (T, C, A, G = 0..3).  A codon with a byte outside
// ACGT is `unknown`; with first_as_m the first residue of a window whose first codon is three ACGT symbols is 'M'.  The protein
// of window k is the plain translation of the bytes window_gather.h writes for window k.
// Written against wave_prims.h only; every collective (the ballot of wave_find) sits in wave-uniform control flow, so the CPU
// fiber harness of tests/emu/ runs this source unchanged.
//
// The walk goes BY OUTPUT RESIDUES, as window_gather.h's goes by output bytes and with the same helpers: granules of 16 residues
// at 16-byte-aligned ABSOLUTE addresses, one owner per granule, a 64-way search for the wave's first window, a galloping walk
// from window to window, one store per granule (single bytes in a partial first / last granule).  The source side is new.
// Inside one window a granule consists of RUNS of codons:
//  - a contiguous run: codons that end before the record does.  The run's first codon sits at granule byte b0, and the 48 source
//    symbols that would fill the whole granule start 3 * b0 symbols in front of it: up to THREE 16-byte loads at those addresses
//    (mirrored, and the 16 bytes reversed in registers, for strand 1), of which only the ones that touch the run are issued.
//    Granule byte b then reads block symbols 3b, 3b + 1, 3b + 2 at positions fixed at compile time: three lookups in a 256-entry
//    class table (0..3, or 4 for any other byte; for strand 1 its composition with `comp`, so both strands agree with the gather
//    on every byte) and one in a 125-entry residue table (index 25 c0 + 5 c1 + c2: `unknown` needs no branch);
//  - a single codon, symbol by symbol: one that crosses the origin, every codon of a record shorter than 3, and the first codon
//    of a window under first_as_m.
// Every 16-byte load goes through ck_compact::load_window and stays inside the payload [bytes + p0, bytes + p1); nothing is
// stored outside [out, out + B); the input is never written.  Output positions, residue counts and B are 64-bit; a record's
// length, a start and a position inside a record are 32-bit.
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "monomer_compact.h"
#include "window_gather.h"

namespace ck_translate {

using ck_compact::u128;
using ck_windows::Window;

constexpr uint32_t TRANSLATE_WAVES = 4, TRANSLATE_STEPS = 4;     // waves per workgroup; steps of 64 granules per wave and tile
constexpr uint32_t WAVE_GRANULES = 64 * TRANSLATE_STEPS, TILE_GRANULES = WAVE_GRANULES * TRANSLATE_WAVES;
constexpr uint32_t TILE_RESIDUES = 16 * TILE_GRANULES;           // 16 Ki residues of output per workgroup and tile
constexpr uint32_t OTHER = 4;                                    // the class of a byte outside ACGT
constexpr uint32_t CLASS_ENTRIES = 256, RESIDUE_ENTRIES = 125;

// The residues window W writes: a third of the bytes the gather writes for it (one or two trailing symbols are ignored)
CK_DEV uint64_t residue_length(const Window& W, const uint64_t* offsets, uint64_t n_records, bool* invalid)
{
    return ck_windows::effective_length(W, offsets, n_records, invalid) / 3;
}

CK_DEV uint32_t class_of(uint32_t byte)
{
    return byte == 'T' ? 0u : byte == 'C' ? 1u : byte == 'A' ? 2u : byte == 'G' ? 3u : OTHER;
}

// The three tables, filled by `threads` workers of which this is number `tid`: cls[0][v] = the class of byte v, cls[1][v] = the
// class of comp[v] (what strand 1 reads where the record holds v), residue[25 c0 + 5 c1 + c2] = aa[16 c0 + 4 c1 + c2], or
// `unknown` where one of the three classes is OTHER.
CK_DEV void fill_tables(uint32_t tid, uint32_t threads, const uint8_t* comp, const uint8_t* aa, uint8_t unknown, uint8_t* cls0, uint8_t* cls1,
                        uint8_t* residue)
{
    for (uint32_t v = tid; v < CLASS_ENTRIES; v += threads) {
        cls0[v] = (uint8_t)class_of(v);
        cls1[v] = (uint8_t)class_of(comp[v]);
    }
    for (uint32_t i = tid; i < RESIDUE_ENTRIES; i += threads) {
        const uint32_t c0 = i / 25, c1 = i / 5 % 5, c2 = i % 5;
        residue[i] = c0 == OTHER || c1 == OTHER || c2 == OTHER ? unknown : aa[16 * c0 + 4 * c1 + c2];
    }
}

struct Translate {
    const uint8_t* bytes;            // the input batch; its payload is bytes[p0 .. p1)
    const uint64_t* offsets;         // n_records + 1 entries
    uint64_t p0, p1;
    const Window* windows;           // m entries; a window with out_offsets[k] == out_offsets[k + 1] is never read
    const uint64_t* out_offsets;     // m + 1 entries in residues, out_offsets[0] = 0, out_offsets[m] = B
    uint64_t m, B;
    const uint8_t *cls0, *cls1;      // the class table of strand 0 and of strand 1, CLASS_ENTRIES each
    const uint8_t* residue;          // RESIDUE_ENTRIES
    uint32_t first_as_m;
    uint8_t* out;
};

CK_DEV uint32_t byte_of(const u128& v, uint32_t k)           // k = 0..15
{
    return (uint32_t)((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xFF);
}

// the 16 bytes of v in reverse order
CK_DEV u128 reverse16(u128 v)
{
    return u128{ __builtin_bswap64(v.hi), __builtin_bswap64(v.lo) };
}

// Granule byte b = the residue of block symbols 3b, 3b + 1, 3b + 2, the block being the 48 symbols c[0], c[1], c[2]
CK_DEV u128 translate48(const u128 (&c)[3], const uint8_t* cls, const uint8_t* residue)
{
    u128 r{ 0, 0 };
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
        const uint32_t k = 3 * b;
        const uint32_t c0 = cls[byte_of(c[k >> 4], k & 15)], c1 = cls[byte_of(c[(k + 1) >> 4], (k + 1) & 15)],
                       c2 = cls[byte_of(c[(k + 2) >> 4], (k + 2) & 15)];
        const uint64_t aa = residue[(c0 * 5 + c1) * 5 + c2];
        if (b < 8) r.lo |= aa << (8 * b); else r.hi |= aa << (8 * (b - 8));
    }
    return r;
}

// One lane's granule: the output residues [q, q + 16), q = its position relative to T.out (negative in a partial first
// granule).  j: a window with out_offsets[j] <= max(q, 0); returns the window the granule's last residue lies in.
CK_DEV uint64_t translate_granule(const Translate& T, int64_t q, uint64_t j)
{
    uint64_t p = q < 0 ? 0 : (uint64_t)q;
    const uint64_t end = (uint64_t)(q + 16) < T.B ? (uint64_t)(q + 16) : T.B;
    u128 acc{ 0, 0 };
    while (p < end) {
        j = ck_compact::lane_seek(T.out_offsets, T.m, j, p);
        const uint64_t o = T.out_offsets[j], o1 = T.out_offsets[j + 1];          // o <= p < o1: the window is valid, its record not empty
        const uint64_t e = o1 < end ? o1 : end;
        const Window W = T.windows[j];
        const uint64_t r0 = T.offsets[W.record];
        const uint32_t n = (uint32_t)(T.offsets[(uint64_t)W.record + 1] - r0);
        const uint8_t* cls = W.strand == 0 ? T.cls0 : T.cls1;
        // residue p is the codon at symbol u of the strand; 3 * (p - o) < the window's length: no overflow
        uint32_t u = ck_windows::cyc_add(W.start < n ? W.start : W.start % n, 3 * (p - o), n);
        bool as_m = T.first_as_m && p == o;
        while (p < e) {
            const uint32_t b0 = (uint32_t)((int64_t)p - q);                      // the run's first residue in the granule
            const uint64_t room = (uint64_t)((n - u) / 3), want = e - p;
            const uint32_t run = as_m ? 0u : (uint32_t)(want < room ? want : room);       // 0 .. 16 codons that end before the record does
            if (run) {
                // block symbol k = strand symbol u - 3 b0 + k, so that granule byte b0 + i reads the run's codon i; chunk i of the
                // block is loaded only where it touches the run's symbols u .. u + 3 run, and then it lies where load_window allows
                u128 c[3];
#pragma unroll
                for (int32_t i = 0; i < 3; ++i) {
                    const int32_t lo = 16 * i - 3 * (int32_t)b0;                  // the chunk's first symbol, relative to u
                    c[i] = u128{ 0, 0 };
                    if (lo < (int32_t)(3 * run) && lo + 16 > 0) {
                        if (W.strand == 0) {
                            c[i] = ck_compact::load_window(T.bytes, T.p0, T.p1, (int64_t)(r0 + u) + lo);
                        } else {
                            // strand symbol x is record byte n-1-x: the chunk's 16 symbols are the 16 bytes that end there, reversed
                            c[i] = reverse16(ck_compact::load_window(T.bytes, T.p0, T.p1, (int64_t)(r0 + (n - 1 - u)) - lo - 15));
                        }
                    }
                }
                const u128 v = translate48(c, cls, T.residue);
                const u128 mk = ck_compact::byte_range(b0, b0 + run);
                acc.lo |= v.lo & mk.lo;
                acc.hi |= v.hi & mk.hi;
                p += run;
                u += 3 * run;
                if (u == n) u = 0;
            } else {
                // one codon, symbol by symbol: it goes round the origin, or it is the window's first under first_as_m
                uint32_t idx = 0, any = 0;
#pragma unroll 1
                for (uint32_t s = 0; s < 3; ++s) {
                    const uint32_t cl = cls[T.bytes[r0 + (W.strand == 0 ? u : n - 1 - u)]];
                    idx = idx * 5 + cl;
                    any |= cl;
                    if (++u == n) u = 0;
                }
                const uint64_t aa = as_m && any < OTHER ? (uint64_t)'M' : (uint64_t)T.residue[idx];       // (classes 0..3 never set bit 2)
                if (b0 < 8) acc.lo |= aa << (8 * b0); else acc.hi |= aa << (8 * (b0 - 8));
                as_m = false;
                p += 1;
            }
        }
    }
    if (q >= 0 && (uint64_t)q + 16 <= T.B) {
        ck::store16(T.out + q, ck::u32x4{ (uint32_t)acc.lo, (uint32_t)(acc.lo >> 32), (uint32_t)acc.hi, (uint32_t)(acc.hi >> 32) });
    } else {
#pragma unroll 1
        for (int64_t x = q < 0 ? 0 : q; x < (int64_t)end; ++x) {        // the first or the last granule of the whole output
            const uint32_t k = (uint32_t)(x - q);
            T.out[x] = (uint8_t)((k < 8 ? acc.lo >> (8 * k) : acc.hi >> (8 * (k - 8))) & 0xFF);
        }
    }
    return j;
}

// Tile `tile` of the output, run by every lane of a workgroup of TRANSLATE_WAVES waves.  *first_window (when given) receives
// the window the wave's search found, for the harness to compare across lanes.
CK_DEV void translate_tile(const Translate& T, uint64_t tile, uint64_t* first_window = nullptr)
{
    if (T.B == 0) return;
    const uint64_t a0 = (uint64_t)(uintptr_t)T.out & 15u;                 // the output's position in its first granule
    const uint64_t n_gran = (a0 + T.B + 15) / 16;
    const uint64_t g0 = tile * TILE_GRANULES + (uint64_t)ck::wave_in_block() * WAVE_GRANULES;
    if (g0 >= n_gran) return;                                            // wave-uniform
    const int64_t q0 = (int64_t)(16 * g0) - (int64_t)a0;
    uint64_t j = ck_compact::wave_find(T.out_offsets, T.m, q0 < 0 ? 0 : (uint64_t)q0);
    if (first_window) *first_window = j;
    const uint32_t lane = ck::lane_id();
#pragma unroll 1
    for (uint32_t s = 0; s < TRANSLATE_STEPS; ++s) {
        const uint64_t g = g0 + 64u * s + lane;
        if (g >= n_gran) break;
        j = translate_granule(T, (int64_t)(16 * g) - (int64_t)a0, j);
    }
}

}  // namespace ck_translate
