// fasta_write.h -- FASTA text from what the device holds: output record k is '>' head label '\n' body '\n', the inverse of
// fasta_device.h.  The head is a span of the input text (circkit_fasta_parse_device's d_head), reached through the kept-record
// map of a compact (d_out_src) when there is one; the label is what `circkit orfs` appends to the id ("_ORF" / "_RC_ORF" and the
// start in decimal: src/orfs.rs:113-114,146-147), made from the window that cut the sequence; the body is a record of a CSR
// batch or the raw span of the text (`uniq` without --canonical-out writes the sequence as it was read: src/uniq.rs:50-61).
// Written against wave_prims.h and monomer_compact.h's helpers only; every collective (the ballot of wave_find) sits in
// wave-uniform control flow, so the CPU fiber harness of tests/emu/ runs this source unchanged.
//
// Three steps.  record_length() per output record: 3 + head + label + body, or 0 for an INVALID record, which is counted and
// of which nothing is dereferenced beyond the entry that proves it invalid.  A saturating scan of the lengths into out_offsets
// (the kernels of circkit_fasta_write.hip; verdict() decides on capacity and overlap).  write_tile() BY OUTPUT BYTES, as
// monomer_compact.h and window_gather.h store: granules of 16 bytes at 16-byte-aligned ABSOLUTE addresses, one owner lane per
// granule, a 64-way search for the wave's first record, a galloping walk from record to record, one 16-byte store per granule
// (single bytes in a partial first / last granule).  Inside one record a granule consists of PIECES: the literal '>', a head
// piece, a label piece, '\n', a body piece, '\n'.  A head or body piece is ONE bounded 16-byte load (ck_compact::load_window)
// at the address that puts the bytes where the granule wants them; the label is made in registers.  The shortest record is 3
// bytes, so a granule may hold five whole records and a part of a sixth: the same loop.
// Nothing is loaded outside [text, text + n_text) or the body payload [body + b0, body + b1); nothing is stored outside
// [out, out + B); neither the text nor the body is written.  Positions, lengths and B are 64-bit.
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "ck_scan.h"
#include "monomer_compact.h"

namespace ck_fwrite {

using ck_compact::u128;

struct Span { uint64_t off, len; };                      // = circkit_fasta_span
struct Label {                                           // = circkit_window; `length` is not read
    uint64_t length;
    uint32_t record, start, strand, reserved;
};

constexpr uint32_t WRITE_WAVES = 4, WRITE_STEPS = 4;     // waves per workgroup; steps of 64 granules per wave and tile
constexpr uint32_t WAVE_GRANULES = 64 * WRITE_STEPS, TILE_GRANULES = WAVE_GRANULES * WRITE_WAVES;
constexpr uint32_t TILE_BYTES = 16 * TILE_GRANULES;      // 16 KiB of output per workgroup and tile
// the scan of the lengths (circkit_fasta_write.hip): records per tile of the scan, tile sums per round of its middle kernel
constexpr uint32_t SCAN_WG = 256, SCAN_ITEMS = 2, SCAN_TILE = SCAN_WG * SCAN_ITEMS;
enum { REFUSED_CAPACITY = 1, REFUSED_OVERLAP = 2 };

// a + b, or ~0 where that does not fit (the scan stays monotone, and no capacity holds ~0)
using ck_scan::sat_add;

// What the records are made of.  Exactly one of raw and body (with body_offsets) is given; src and labels may be null.
struct Source {
    const uint8_t* text; uint64_t n_text;
    const Span* head; const Span* raw; uint64_t n_heads;
    const uint64_t* src; uint64_t n_src;
    const Label* labels;
    const uint8_t* body; const uint64_t* body_offsets;
    uint64_t b0, b1;                                     // the body payload is body[b0 .. b1): body_offsets[0], body_offsets[n_out]
};

struct Parts {                                           // one valid record
    uint64_t head_off, head_len;                         // in the text
    uint64_t body_off, body_len;                         // in the body payload, or in the text (raw)
    uint32_t label_len, start, strand;
};

// overflow-safe: the span lies in [0, n)
CK_DEV bool span_inside(const Span& s, uint64_t n) { return !(s.off > n || s.len > n - s.off); }

CK_DEV uint32_t decimal_digits(uint32_t v)               // 1 .. 10: Rust's u32::to_string
{
    uint32_t d = 1;
    while (v >= 10) { v /= 10; ++d; }
    return d;
}

// Record k's parts; false for an INVALID record: a label with a strand other than 0 / 1 or a reserved word in use, a record
// beyond the map (i_k >= n_src), a header beyond the spans (h_k >= n_heads), a head or raw span that does not lie in the text,
// a body range that decreases or leaves [b0, b1).  Each entry is checked before anything it names is read.
CK_DEV bool resolve(const Source& S, uint64_t k, Parts* P)
{
    uint64_t i = k;
    P->label_len = 0; P->start = 0; P->strand = 0;
    if (S.labels) {
        const Label L = S.labels[k];
        if (L.strand > 1 || L.reserved != 0) return false;
        i = L.record;
        P->start = L.start; P->strand = L.strand;
        P->label_len = (L.strand ? 7u : 4u) + decimal_digits(L.start);
    }
    if (i >= S.n_src) return false;
    const uint64_t h = S.src ? S.src[i] : i;
    if (h >= S.n_heads) return false;
    const Span H = S.head[h];
    if (!span_inside(H, S.n_text)) return false;
    P->head_off = H.off; P->head_len = H.len;
    if (S.body) {
        const uint64_t o0 = S.body_offsets[k], o1 = S.body_offsets[k + 1];
        if (o0 < S.b0 || o1 > S.b1 || o1 < o0) return false;
        P->body_off = o0; P->body_len = o1 - o0;
    } else {
        const Span R = S.raw[h];
        if (!span_inside(R, S.n_text)) return false;
        P->body_off = R.off; P->body_len = R.len;
    }
    return true;
}

// The bytes record k writes: '>' head label '\n' body '\n', or 0 for an invalid record, which sets *invalid.
CK_DEV uint64_t record_length(const Source& S, uint64_t k, bool* invalid)
{
    Parts P;
    *invalid = !resolve(S, k, &P);
    if (*invalid) return 0;
    return sat_add(sat_add(3ull + P.label_len, P.head_len), P.body_len);
}

// The refusals of a write whose lengths add up to `total`: a total beyond the capacity, and an output [out, out + total) that
// overlaps the text or the body payload.  out may be null where only the offsets are wanted.
CK_DEV uint32_t verdict(uint64_t total, uint64_t capacity, const uint8_t* text, uint64_t n_text, const uint8_t* body, uint64_t b0, uint64_t b1,
                        const uint8_t* out)
{
    if (total > capacity || total == ~0ull) return REFUSED_CAPACITY;
    if (!total || !out) return 0;
    const uintptr_t lo = (uintptr_t)out, hi = lo + total;
    if (n_text && lo < (uintptr_t)text + n_text && (uintptr_t)text < hi) return REFUSED_OVERLAP;
    if (body && b1 > b0 && lo < (uintptr_t)body + b1 && (uintptr_t)body + b0 < hi) return REFUSED_OVERLAP;
    return 0;
}

// ---- the label in registers: up to 7 tag bytes and 10 digits, byte t of the label = byte t of {w0, w1, w2} ----
struct LabelBytes { uint64_t w0, w1, w2; };

CK_DEV LabelBytes make_label(uint32_t strand, uint32_t start, uint32_t label_len)
{
    LabelBytes L{ strand ? 0x46524F5F43525Full : 0x46524F5Full, 0, 0 };      // "_RC_ORF" / "_ORF", first byte lowest
    uint32_t pos = label_len, v = start;
    do {                                                                     // the digits from the right
        --pos;
        const uint64_t d = (uint64_t)('0' + v % 10);
        if (pos < 8) L.w0 |= d << (8 * pos);
        else if (pos < 16) L.w1 |= d << (8 * (pos - 8));
        else L.w2 |= d << (8 * (pos - 16));
        v /= 10;
    } while (v);
    return L;
}

CK_DEV uint64_t label_byte(const LabelBytes& L, uint32_t t)
{
    return ((t < 8 ? L.w0 >> (8 * t) : t < 16 ? L.w1 >> (8 * (t - 8)) : L.w2 >> (8 * (t - 16)))) & 0xFF;
}

// byte k of the granule (0 .. 15, still zero) = b
CK_DEV void put_byte(u128& acc, uint32_t k, uint64_t b)
{
    if (k < 8) acc.lo |= b << (8 * k); else acc.hi |= b << (8 * (k - 8));
}

struct Write {
    Source S;
    const uint64_t* out_offsets;     // m + 1 entries, out_offsets[0] = 0, out_offsets[m] = B
    uint64_t m, B;
    uint8_t* out;
};

// One lane's granule: the output bytes [q, q + 16), q = its position relative to W.out (negative in a partial first granule).
// j: a record with out_offsets[j] <= max(q, 0); returns the record the granule's last byte lies in.
CK_DEV uint64_t write_granule(const Write& W, int64_t q, uint64_t j)
{
    uint64_t p = q < 0 ? 0 : (uint64_t)q;
    const uint64_t end = (uint64_t)(q + 16) < W.B ? (uint64_t)(q + 16) : W.B;
    u128 acc{ 0, 0 };
    while (p < end) {
        j = ck_compact::lane_seek(W.out_offsets, W.m, j, p);
        const uint64_t o = W.out_offsets[j], o1 = W.out_offsets[j + 1];      // o <= p < o1: the record is valid
        const uint64_t e = o1 < end ? o1 : end;
        Parts P;
        (void)resolve(W.S, j, &P);
        const uint64_t nl1 = 1 + P.head_len + P.label_len, nl2 = o1 - o - 1;  // where the record's two '\n' are
        while (p < e) {
            const uint64_t rel = p - o, want = e - p;                        // want = 1 .. 16
            const uint32_t g = (uint32_t)((int64_t)p - q);                   // the piece's first byte in the granule
            uint32_t len = 1;
            if (rel == 0) {
                put_byte(acc, g, '>');
            } else if (rel <= P.head_len) {
                // granule byte g + i = text byte head_off + rel - 1 + i: the 16 bytes that start g in front of that byte
                const uint64_t room = P.head_len - (rel - 1);
                len = (uint32_t)(want < room ? want : room);
                const u128 v = ck_compact::load_window(W.S.text, 0, W.S.n_text, (int64_t)(P.head_off + rel - 1) - (int64_t)g);
                const u128 mk = ck_compact::byte_range(g, g + len);
                acc.lo |= v.lo & mk.lo;
                acc.hi |= v.hi & mk.hi;
            } else if (rel < nl1) {
                const uint32_t t = (uint32_t)(rel - 1 - P.head_len), room = P.label_len - t;
                len = want < room ? (uint32_t)want : room;
                const LabelBytes L = make_label(P.strand, P.start, P.label_len);
#pragma unroll 1
                for (uint32_t i = 0; i < len; ++i) put_byte(acc, g + i, label_byte(L, t + i));
            } else if (rel == nl1 || rel == nl2) {
                put_byte(acc, g, '\n');
            } else {
                const uint64_t t = rel - nl1 - 1, room = P.body_len - t;
                len = (uint32_t)(want < room ? want : room);
                const int64_t at = (int64_t)(P.body_off + t) - (int64_t)g;
                const u128 v = W.S.body ? ck_compact::load_window(W.S.body, W.S.b0, W.S.b1, at) : ck_compact::load_window(W.S.text, 0, W.S.n_text, at);
                const u128 mk = ck_compact::byte_range(g, g + len);
                acc.lo |= v.lo & mk.lo;
                acc.hi |= v.hi & mk.hi;
            }
            p += len;
        }
    }
    if (q >= 0 && (uint64_t)q + 16 <= W.B) {
        ck::store16(W.out + q, ck::u32x4{ (uint32_t)acc.lo, (uint32_t)(acc.lo >> 32), (uint32_t)acc.hi, (uint32_t)(acc.hi >> 32) });
    } else {
#pragma unroll 1
        for (int64_t x = q < 0 ? 0 : q; x < (int64_t)end; ++x) {        // the first or the last granule of the whole output
            const uint32_t k = (uint32_t)(x - q);
            W.out[x] = (uint8_t)((k < 8 ? acc.lo >> (8 * k) : acc.hi >> (8 * (k - 8))) & 0xFF);
        }
    }
    return j;
}

// Tile `tile` of the output, run by every lane of a workgroup of WRITE_WAVES waves.  *first_record (when given) receives the
// record the wave's search found, for the harness to compare across lanes.
CK_DEV void write_tile(const Write& W, uint64_t tile, uint64_t* first_record = nullptr)
{
    if (W.B == 0) return;
    const uint64_t a0 = (uint64_t)(uintptr_t)W.out & 15u;                 // the output's position in its first granule
    const uint64_t n_gran = (a0 + W.B + 15) / 16;
    const uint64_t g0 = tile * TILE_GRANULES + (uint64_t)ck::wave_in_block() * WAVE_GRANULES;
    if (g0 >= n_gran) return;                                            // wave-uniform
    const int64_t q0 = (int64_t)(16 * g0) - (int64_t)a0;
    uint64_t j = ck_compact::wave_find(W.out_offsets, W.m, q0 < 0 ? 0 : (uint64_t)q0);
    if (first_record) *first_record = j;
    const uint32_t lane = ck::lane_id();
#pragma unroll 1
    for (uint32_t s = 0; s < WRITE_STEPS; ++s) {
        const uint64_t g = g0 + 64u * s + lane;
        if (g >= n_gran) break;
        j = write_granule(W, (int64_t)(16 * g) - (int64_t)a0, j);
    }
}

}  // namespace ck_fwrite
