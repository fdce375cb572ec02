// fasta_device.h -- FASTA text on the device: text[0, n) becomes the normalized CSR batch that ckhost::parse_chunk
// (fasta_host.cpp) makes of it on the host, byte for byte: seq_io 0.3.2's record boundaries and needletail 0.5.1
// normalize(_, false) through the table of ckhost::normalize_lut().
// Written against wave_prims.h only; every collective (ballot, shfl, wave_sum_u64, block_barrier) sits in control flow that is
// uniform over the wave -- the barriers over the workgroup -- so the CPU fiber harness of tests/emu/ runs this source unchanged.
//
// Per byte i of [p0, limit) (resolve_bounds; a byte outside that range is nothing at all):
//   start(i)  i == p0, or text[i] == '>' behind text[i - 1] == '\n'
//   nl(i)     text[i] == '\n' and not a start
//   keep(i)   the table's entry for text[i] is not 0
// and one state that runs along the text: a start sets HEADER, a newline sets SEQ, anything else leaves it.  A byte is written
// iff keep(i) and the state behind it is SEQ; its record is the number of starts at or before it, less one.  The state is a
// last-writer-wins scan, the output position a sum scan that depends on it, so a tile of TILE_BYTES is summarized as
//   kind     its last event (ST_PASS: it has none and hands the state on unchanged)
//   starts   its record starts
//   inherit  its keep bytes in front of its first event: written iff the tile BEGINS in a sequence, which only the scan knows
//   kept     its keep bytes behind its first event that are written
// One workgroup scans the summaries (the .hip; next_state / tile_kept below are its two rules), then apply_tile runs every tile
// again with its three prefixes known.  A header or a line may be as long as it likes: a tile without an event is ST_PASS.
//
// apply_tile packs a tile's written bytes in LDS at the position they have in the output modulo 16, so that the LDS image and
// the output share their 16-byte granules.  Every granule that lies wholly inside the tile's output range is ONE aligned
// 16-byte store from one lane; the (at most two) granules a tile shares with its neighbours are stored as single bytes, each
// byte by the tile that owns it: no granule is ever read back, and no two workgroups store to the same byte.
// Every load of the text goes through ck_compact::load_window over [text, text + n) or is a single guarded byte; nothing is
// stored outside [out, out + payload); the text is never written.  All positions and counts are 64-bit.
#pragma once
#include <stdint.h>
#include "wave_prims.h"
#include "monomer_compact.h"

namespace ck_fasta {

using ck_compact::u128;

constexpr uint32_t WAVES = 4, WG = 64 * WAVES;            // a workgroup: one lane per 16 bytes of its tile
constexpr uint32_t TILE_BYTES = 16 * WG;                  // 4 KiB of text per workgroup and tile
constexpr uint32_t SCAN_WG = 256;                         // summaries per round of the scan over them
enum { ST_PASS = 0, ST_HEADER = 1, ST_SEQ = 2 };
enum { REFUSED_CAPACITY = 1, REFUSED_OVERLAP = 2, REFUSED_FORMAT = 3 };

struct Span { uint64_t off, len; };                       // = circkit_fasta_span
struct Text { const uint8_t* text; uint64_t n, p0, limit; };
struct Summary { uint32_t kind, starts, inherit, kept; };
struct Prefix { uint64_t records, bytes, state; };        // in front of a tile: its first record start's number, its first byte's position

struct Shared {                                           // the LDS of one workgroup
    alignas(16) uint8_t out[TILE_BYTES + 16];
    uint8_t lut[256];
    uint32_t wave_kind[WAVES];
    uint64_t wave_count[WAVES];
};

CK_DEV uint32_t byte_at(const u128& v, uint32_t k) { return (uint32_t)((k < 8 ? v.lo >> (8 * k) : v.hi >> (8 * (k - 8))) & 0xFF); }
CK_DEV uint32_t below(uint32_t k) { return (1u << k) - 1u; }                 // the bits under bit k, k = 0..15

// ---- p0 and limit ----
// The 16 bytes at pos < n: *first_body = the first byte that is neither '\n' nor '\r' (a minimum), *last_candidate = the last
// '>' behind a '\n' (a maximum; 0: none, the first candidate there can be is 1).
CK_DEV void scan_bounds16(const uint8_t* text, uint64_t n, uint64_t pos, uint64_t* first_body, uint64_t* last_candidate)
{
    const u128 v = ck_compact::load_window(text, 0, n, (int64_t)pos);
    const uint32_t cnt = n - pos < 16 ? (uint32_t)(n - pos) : 16u;
    uint32_t prev = pos ? text[pos - 1] : 0u;
#pragma unroll 1
    for (uint32_t k = 0; k < cnt; ++k) {
        const uint32_t b = byte_at(v, k);
        if (b != '\n' && b != '\r' && pos + k < *first_body) *first_body = pos + k;
        if (b == '>' && prev == '\n' && pos + k > *last_candidate) *last_candidate = pos + k;
        prev = b;
    }
}

// With first_chunk p0 is the first byte that is no line end, and a p0 < n that is not '>' is the format error; without, 0.
// With final_chunk limit = n; without, the last record start beyond p0 (a candidate: p0 is at most the first of them), or p0.
// After an error limit = p0: no byte is anything.
CK_DEV Text resolve_bounds(const uint8_t* text, uint64_t n, uint64_t first_body, uint64_t last_candidate, bool first_chunk, bool final_chunk,
                           bool* error)
{
    Text T{ text, n, 0, 0 };
    T.p0 = first_chunk ? (first_body < n ? first_body : n) : 0;
    *error = first_chunk && T.p0 < n && text[T.p0] != '>';
    T.limit = final_chunk ? n : (last_candidate > T.p0 ? last_candidate : T.p0);
    if (*error) T.limit = T.p0;
    return T;
}

// ---- one lane's 16 bytes ----
struct Lane {
    u128 v;
    uint32_t start, nl, keep;        // one bit per byte
};

CK_DEV Lane classify(const Text& T, uint64_t pos, const uint8_t* lut)
{
    Lane L{ { 0, 0 }, 0, 0, 0 };
    if (pos >= T.limit || pos + 16 <= T.p0) return L;     // (limit <= n: the load below starts inside the text)
    L.v = ck_compact::load_window(T.text, 0, T.n, (int64_t)pos);
    uint32_t prev = pos ? T.text[pos - 1] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = pos + k;
        const uint32_t b = byte_at(L.v, k), bit = 1u << k;
        if (i >= T.p0 && i < T.limit) {
            if (i == T.p0 || (b == '>' && prev == '\n')) L.start |= bit;
            else if (b == '\n') L.nl |= bit;
            if (lut[b]) L.keep |= bit;
        }
        prev = b;
    }
    return L;
}

CK_DEV uint32_t lane_kind(const Lane& L)
{
    const uint32_t ev = L.start | L.nl;
    if (!ev) return ST_PASS;
    return (L.start >> (31 - ck::clz32(ev))) & 1u ? ST_HEADER : ST_SEQ;
}

// Walks the lane's bytes from state s (ST_PASS: the state at the tile's start, which is not known).  *kept = the bytes that
// are written, *inherit = the keep bytes still in ST_PASS, *closing = the newlines that end a header.
CK_DEV void walk(const Lane& L, uint32_t s, uint32_t* kept, uint32_t* inherit, uint32_t* closing)
{
    uint32_t km = 0, pm = 0, cm = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        const uint32_t bit = 1u << k;
        if (L.start & bit) s = ST_HEADER;
        else if (L.nl & bit) { if (s == ST_HEADER) cm |= bit; s = ST_SEQ; }
        if (L.keep & bit) { if (s == ST_SEQ) km |= bit; else if (s == ST_PASS) pm |= bit; }
    }
    *kept = km; *inherit = pm; *closing = cm;
}

// The state in front of this lane's bytes: the last event of the lanes below it, of the waves below its wave, or tile_in.
// *tile_kind = the tile's last event.  Ends behind a barrier; the caller owes one before S.wave_kind is written again.
CK_DEV uint32_t state_before(uint32_t kind, uint32_t tile_in, Shared& S, uint32_t* tile_kind)
{
    const uint32_t lane = ck::lane_id(), wave = ck::wave_in_block();
    const uint64_t bh = ck::ballot(kind == ST_HEADER), bq = ck::ballot(kind == ST_SEQ);
    const uint64_t any = bh | bq;
    if (lane == 0) S.wave_kind[wave] = any ? ((bq >> (63 - __builtin_clzll(any))) & 1u ? ST_SEQ : ST_HEADER) : ST_PASS;
    ck::block_barrier();
    uint32_t in = tile_in, all = ST_PASS;
    for (uint32_t w = 0; w < WAVES; ++w) {
        const uint32_t k = S.wave_kind[w];
        if (k && w < wave) in = k;
        if (k) all = k;
    }
    *tile_kind = all;
    const uint64_t lower = any & ((1ull << lane) - 1ull);
    if (!lower) return in;
    return (bq >> (63 - __builtin_clzll(lower))) & 1u ? ST_SEQ : ST_HEADER;
}

// ---- the summary of tile `tile`, run by every lane of a workgroup of WAVES waves (S.lut filled, a barrier behind it) ----
CK_DEV void summarize_tile(const Text& T, uint64_t tile, Shared& S, Summary* out)
{
    const uint32_t lane = ck::lane_id(), wave = ck::wave_in_block();
    const uint64_t pos = tile * TILE_BYTES + 16ull * (wave * 64u + lane);
    const Lane L = classify(T, pos, S.lut);
    uint32_t kind, km, pm, cm;
    const uint32_t s = state_before(lane_kind(L), ST_PASS, S, &kind);
    walk(L, s, &km, &pm, &cm);
    // three counts of at most 16 a lane in one word: 20 bits each hold a wave's sum and a workgroup's
    const uint64_t sum = ck::wave_sum_u64((uint64_t)ck::popc32(pm) | (uint64_t)ck::popc32(km) << 20 | (uint64_t)ck::popc32(L.start) << 40);
    if (lane == 0) S.wave_count[wave] = sum;
    ck::block_barrier();
    if (wave == 0 && lane == 0) {
        uint64_t t = 0;
        for (uint32_t w = 0; w < WAVES; ++w) t += S.wave_count[w];
        *out = Summary{ kind, (uint32_t)(t >> 40), (uint32_t)(t & 0xFFFFF), (uint32_t)((t >> 20) & 0xFFFFF) };
    }
    ck::block_barrier();
}

// ---- the scan's two rules ----
CK_DEV uint32_t next_state(uint32_t in, uint32_t kind) { return kind ? kind : in; }
CK_DEV uint32_t tile_kept(const Summary& s, uint32_t in) { return s.kept + (in == ST_SEQ ? s.inherit : 0u); }

// The verdict on the totals: more records or bytes than the caller's buffers hold, or an output [out, out + bytes) that
// overlaps the text.
CK_DEV uint32_t verdict(uint64_t records, uint64_t bytes, uint64_t record_capacity, uint64_t byte_capacity, const uint8_t* text, uint64_t n,
                        const uint8_t* out)
{
    if (records > record_capacity || bytes > byte_capacity) return REFUSED_CAPACITY;
    if (bytes && n) {
        const uintptr_t in_lo = (uintptr_t)text, in_hi = in_lo + n, out_lo = (uintptr_t)out, out_hi = out_lo + bytes;
        if (out_lo < in_hi && in_lo < out_hi) return REFUSED_OVERLAP;
    }
    return 0;
}

// ---- apply ----
struct Apply {
    Text T;
    const Prefix* prefix;            // per tile
    uint8_t* out;                    // the payload
    uint64_t* offsets;               // offsets[r] of every record start; offsets[n_records] is the scan's
    Span* head;                      // head[r].off, or null (both or neither)
    Span* raw;                       // raw[r].off of every record whose header ends in a newline
};

CK_DEV void apply_tile(const Apply& A, uint64_t tile, Shared& S)
{
    const uint32_t lane = ck::lane_id(), wave = ck::wave_in_block(), tid = wave * 64u + lane;
    const uint64_t pos = tile * TILE_BYTES + 16ull * tid;
    const Prefix P = A.prefix[tile];
    const Lane L = classify(A.T, pos, S.lut);
    uint32_t kind, km, pm, cm;
    const uint32_t s = state_before(lane_kind(L), (uint32_t)P.state, S, &kind);
    walk(L, s, &km, &pm, &cm);
    // written bytes (low half) and record starts (high half) in front of this lane: a scan over the wave, then over the waves
    const uint32_t mine = (uint32_t)ck::popc32(km) | (uint32_t)ck::popc32(L.start) << 16;
    uint32_t x = mine;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = ck::shfl(x, lane >= d ? lane - d : lane);
        if (lane >= d) x += o;
    }
    const uint32_t wave_total = ck::shfl(x, 63);
    if (lane == 0) S.wave_count[wave] = wave_total;
    ck::block_barrier();
    uint32_t base = 0, all = 0;
    for (uint32_t w = 0; w < WAVES; ++w) {
        const uint32_t c = (uint32_t)S.wave_count[w];
        if (w < wave) base += c;
        all += c;
    }
    const uint32_t before = base + x - mine;
    const uint32_t kept0 = before & 0xFFFFu, starts0 = before >> 16, K = all & 0xFFFFu;
    for (uint32_t m = L.start; m; m &= m - 1) {
        const uint32_t k = (uint32_t)ck::ffs32(m);
        const uint64_t r = P.records + starts0 + (uint32_t)ck::popc32(L.start & below(k));
        A.offsets[r] = P.bytes + kept0 + (uint32_t)ck::popc32(km & below(k));
        if (A.head) A.head[r].off = pos + k + 1;
    }
    if (A.raw) {
        for (uint32_t m = cm; m; m &= m - 1) {
            const uint32_t k = (uint32_t)ck::ffs32(m);
            const uint64_t seen = P.records + starts0 + (uint32_t)ck::popc32(L.start & below(k));     // starts in front of the newline: >= 1
            if (seen) A.raw[seen - 1].off = pos + k + 1;
        }
    }
    // the tile's bytes, packed where the output's granules want them
    const uint32_t a0 = (uint32_t)(((uintptr_t)A.out + P.bytes) & 15u);
    for (uint32_t m = km; m; m &= m - 1) {
        const uint32_t k = (uint32_t)ck::ffs32(m);
        S.out[a0 + kept0 + (uint32_t)ck::popc32(km & below(k))] = S.lut[byte_at(L.v, k)];
    }
    ck::block_barrier();
    if (K) {
        uint8_t* const dst = A.out + P.bytes;                                  // LDS byte a0 + x = dst[x]
        const uint32_t n_gran = (a0 + K + 15) / 16;
#pragma unroll 1
        for (uint32_t g = tid; g < n_gran; g += WG) {
            const uint32_t lo = 16 * g, hi = lo + 16;
            if (lo >= a0 && hi <= a0 + K) {
                ck::store16(dst + (lo - a0), ck::lds_load16((const uint32_t*)(const void*)(S.out + lo)));
            } else {
#pragma unroll 1
                for (uint32_t b = lo < a0 ? a0 : lo; b < hi && b < a0 + K; ++b) dst[b - a0] = S.out[b];
            }
        }
    }
    ck::block_barrier();
}

// ---- the spans of record r, once apply has left head[r].off = S + 1 and, for a header that ends in a newline at e,
// raw[r].off = e + 1.  last_has_end: the text's last state is ST_SEQ.  Writes head[r].len, raw[r].off and raw[r].len only, so
// the lane of record r - 1 may read head[r].off meanwhile.
CK_DEV void finish_spans(const Text& T, uint64_t r, uint64_t n_records, bool last_has_end, Span* head, Span* raw)
{
    const uint64_t S = head[r].off - 1;
    const uint64_t next = r + 1 < n_records ? head[r + 1].off - 1 : T.limit;
    // a next start at S + 1 stands behind the '\n' that is text[S] itself: a start that is no '>' (p0 = 0 without first_chunk)
    const bool has_end = r + 1 < n_records ? next > S + 1 : last_has_end;
    const uint64_t s0 = has_end ? raw[r].off : next;
    const uint64_t e = has_end ? s0 - 1 : next;
    uint64_t hlen = e - (S + 1);
    if (hlen && T.text[S + hlen] == '\r') --hlen;
    uint64_t rlen = next - s0;
    if (rlen && T.text[s0 + rlen - 1] == '\n') --rlen;
    if (rlen && T.text[s0 + rlen - 1] == '\r') --rlen;
    head[r].len = hlen;
    raw[r].off = s0;
    raw[r].len = rlen;
}

}  // namespace ck_fasta
