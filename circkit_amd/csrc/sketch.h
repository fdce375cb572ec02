// sketch.h -- the cyclic k-mer MinHash sketch of every record of a device batch, and the comparison of two sketches: the "sketches
// of circular records" section of include/circkit.h, which is the definition.  A record of n >= k symbols has n cyclic k-mers; one
// whose k bytes are all of A C G T is packed to 2k bits forward (f) and as its reverse complement (r), h = fmix64(min(f, r) ^ seed),
// and bin h >> (64 - log2_bins) of the record's row keeps the smallest h it saw (EMPTY where none).  The row is a function of the
// multiset of canonical cyclic k-mers: the same for every rotation, for the reverse complement and for the record twice in a row.
// Written against wave_prims.h only; every collective (wave_sync, wave_sum_u64, ballot) sits in wave-uniform control flow, so the
// CPU fiber harness of tests/emu/ runs this source unchanged.
//
// One routine does the work, sketch_span: the starts [s0, s0 + cnt) of one record, run by one wave with a slice of LDS of its own.
//  - pack: the cnt + k - 1 symbols (s0 + i) mod n go to LDS at 2 bits each, 32 to a 64-bit word with the first symbol on top, and a
//    bit per symbol says "not ACGT".  Lane l packs words l, l + 64, ..: two 16-byte loads where the word's 32 symbols lie in the
//    record without crossing its end, single bytes otherwise.  The wrapped symbols are appended, so no k-mer needs a modulo.
//  - hash: lane l takes the starts l, l + 64, ..  f is the top 2k bits of the two words at bit 2p; r is the complement, bit-reversed,
//    with the bits of every pair swapped back; validity is k bits of the mask.  There is no rolling state and no warm-up.
//  - bins: a row of 2^log2_bins 64-bit words in LDS, EMPTY at first, updated by the 64-bit LDS minimum.
// A record of up to SKETCH_SEG symbols is one span and its row is stored with plain coalesced stores (short_record).  A longer one
// gets an EMPTY row there and goes to a list; long_block then runs its spans of SKETCH_SEG starts on as many waves as it has
// spans, and each merges its bins that are not EMPTY into the row by the 64-bit global minimum.  Minimum and sum commute, so
// neither the list's order nor the order of the merges reaches the result.
// The anchors (where each bin's k-mer starts, and the strand of its canonical form: the "pre-alignment" section) are the same build
// with one more sweep over the packed starts once the bins are final; see "anchors" below.  sketch_span is sketch_span_t<false>.
// Nothing is read outside the records' bytes and the offsets; a record of 2^31 symbols or more is never dereferenced.
#pragma once
#include <stdint.h>
#include "wave_prims.h"

namespace ck_sketch {

constexpr uint32_t SKETCH_SEG = 4096;                    // starts per span: a record up to this long is one span
constexpr uint32_t SKETCH_WAVES = 4;                     // waves per workgroup, each with a slice of LDS of its own
constexpr uint32_t K_MIN = 4, K_MAX = 32, LOG2_BINS_MIN = 4, LOG2_BINS_MAX = 10;
constexpr uint64_t EMPTY = ~0ull;
constexpr uint64_t TOO_LONG = 1ull << 31;                // a record of this many symbols is not processed
// per wave: the packed symbols (one word more than the span fills: the hash reads two), the mask, the bins
constexpr uint32_t PACK_WORDS = (SKETCH_SEG + K_MAX - 1 + 31) / 32 + 1;
constexpr uint32_t MASK_WORDS = (PACK_WORDS + 3) & ~3u;  // (32-bit words; rounded so that the bins start at a multiple of 16 bytes)
enum { T_VALID, T_UNPROCESSED, T_LONG, T_WORDS };        // the totals of a sketch, in device memory
enum { REC_DONE, REC_LONG, REC_TOO_LONG };

// The 64-bit atomics the unit needs.  The fibers of the CPU harness do not preempt each other between collectives, so a plain
// compare-and-store is the same there.
#ifdef CK_WAVE_PRIMS_OVERRIDE
CK_DEV void lds_min_u64(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
CK_DEV void global_min_u64(uint64_t* p, uint64_t v) { if (v < *p) *p = v; }
CK_DEV uint64_t global_add_u64(uint64_t* p, uint64_t v) { const uint64_t o = *p; *p = o + v; return o; }
CK_DEV void global_min_u32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
#else
CK_DEV void lds_min_u64(uint64_t* p, uint64_t v) { atomicMin((unsigned long long*)p, (unsigned long long)v); }      // ds_min_u64
CK_DEV void global_min_u64(uint64_t* p, uint64_t v) { atomicMin((unsigned long long*)p, (unsigned long long)v); }
CK_DEV uint64_t global_add_u64(uint64_t* p, uint64_t v) { return atomicAdd((unsigned long long*)p, (unsigned long long)v); }
CK_DEV void global_min_u32(uint32_t* p, uint32_t v) { atomicMin(p, v); }
#endif

constexpr uint32_t lds_words(uint32_t log2_bins) { return PACK_WORDS + MASK_WORDS / 2 + (1u << log2_bins); }           // 64-bit words per wave

struct Lds {
    uint64_t* pack;      // PACK_WORDS
    uint32_t* mask;      // MASK_WORDS
    uint64_t* bins;      // 1 << log2_bins
};
CK_DEV Lds lds_of(uint64_t* slice) { return Lds{ slice, (uint32_t*)(slice + PACK_WORDS), slice + PACK_WORDS + MASK_WORDS / 2 }; }

struct Sketch {
    const uint8_t* bytes;
    const uint64_t* offsets;         // n_records + 1 entries
    uint64_t n_records;
    uint32_t k, log2_bins;
    uint64_t seed;
    uint64_t* out;                   // n_records << log2_bins
    uint32_t* out_count;             // n_records, or null
    uint64_t* long_list;             // n_records: the records of more than SKETCH_SEG symbols, in any order
    uint64_t* totals;                // T_WORDS
};

// MurmurHash3's 64-bit finalizer
CK_DEV uint64_t fmix64(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

CK_DEV uint64_t rev64(uint64_t v) { return ((uint64_t)ck::bitrev((uint32_t)v) << 32) | ck::bitrev((uint32_t)(v >> 32)); }

// symbol j (0..31) of a word: its code on top-down bit pair j, its "not ACGT" on mask bit j
CK_DEV void add_symbol(uint32_t byte, uint32_t j, uint64_t& code, uint32_t& bad)
{
    const uint32_t t = (byte >> 1) & 3u, c = t ^ (t >> 1);               // A C G T = 0 1 2 3 (bits 1 and 2 of the ASCII code: 0 1 3 2)
    code |= (uint64_t)c << (62u - 2u * j);
    bad |= (byte != ((0x54474341u >> (8u * c)) & 0xFFu) ? 1u : 0u) << j;   // "ACGT"[c]
}

CK_DEV void add_dword(uint32_t w, uint32_t j, uint64_t& code, uint32_t& bad)
{
    add_symbol(w & 0xFF, j, code, bad);
    add_symbol((w >> 8) & 0xFF, j + 1, code, bad);
    add_symbol((w >> 16) & 0xFF, j + 2, code, bad);
    add_symbol(w >> 24, j + 3, code, bad);
}

// The pack of a span: the cnt + k - 1 symbols (s0 + i) mod n of rec[0 .. n) into L.pack and L.mask (cnt > 0).
CK_DEV void pack_span(const uint8_t* rec, uint32_t n, uint32_t s0, uint32_t T, uint32_t words, const Lds& L)
{
    for (uint32_t w = ck::lane_id(); w <= words; w += 64) {              // (word `words` is the zero word the last k-mers read as their second)
        uint64_t code = 0;
        uint32_t bad = 0;
        if (w < words) {
            uint32_t idx = s0 + 32 * w;                                  // < n + k - 1 <= 2n - 1
            if (idx >= n) idx -= n;
            if (idx + 32 <= n) {
                // the word's 32 symbols lie in the record; the ones past the span's end are read and never used
                const ck::u32x4 a = ck::load16(rec + idx), b = ck::load16(rec + idx + 16);
                add_dword(a.x, 0, code, bad); add_dword(a.y, 4, code, bad); add_dword(a.z, 8, code, bad); add_dword(a.w, 12, code, bad);
                add_dword(b.x, 16, code, bad); add_dword(b.y, 20, code, bad); add_dword(b.z, 24, code, bad); add_dword(b.w, 28, code, bad);
            } else {
                const uint32_t left = T - 32 * w < 32 ? T - 32 * w : 32;
#pragma unroll 1
                for (uint32_t j = 0; j < left; ++j) {
                    add_symbol(rec[idx], j, code, bad);
                    if (++idx == n) idx = 0;
                }
            }
        }
        L.pack[w] = code;
        L.mask[w] = bad;
    }
}

// The k-mer at start p of the packed span: whether it is valid, and then its h and o = (r < f), the strand of its canonical form.
CK_DEV bool kmer_at(const Lds& L, uint32_t p, uint32_t kmask, uint32_t down, uint64_t seed, uint64_t& h, uint32_t& o)
{
    const uint32_t q = p >> 5, sh = p & 31;
    const uint64_t m = (((uint64_t)L.mask[q + 1] << 32) | L.mask[q]) >> sh;
    if (((uint32_t)m & kmask) != 0) return false;                        // a symbol outside ACGT among the k
    const uint64_t hi = L.pack[q], lo = L.pack[q + 1];
    const uint64_t g = sh ? (hi << (2 * sh)) | (lo >> (64 - 2 * sh)) : hi;           // the k-mer on top, whatever follows it below
    const uint64_t f = g >> down;
    // complement, all 64 bits reversed (the k-mer's pairs arrive at the bottom in reverse order, each pair's bits swapped),
    // the pairs' bits swapped back, the 2k bits kept
    uint64_t r = rev64(~g);
    r = ((r & 0x5555555555555555ull) << 1) | ((r >> 1) & 0x5555555555555555ull);
    r = (r << down) >> down;
    h = fmix64((f < r ? f : r) ^ seed);
    o = r < f;
    return true;
}

constexpr uint32_t ANCHOR_NONE = 0xFFFFFFFFu;

// The anchors of a packed span whose bins are final in L.bins: a start whose h equals its bin (and is not EMPTY) brings 2p + o,
// p its start in the record, to anchors[bin] by the 32-bit LDS minimum: the smallest start wins.
CK_DEV void anchor_sweep(uint32_t k, uint32_t log2_bins, uint64_t seed, uint32_t s0, uint32_t cnt, const Lds& L, uint32_t* anchors)
{
    const uint32_t kmask = k == 32 ? ~0u : (1u << k) - 1u, down = 64 - 2 * k, bin_shift = 64 - log2_bins;
    for (uint32_t p = ck::lane_id(); p < cnt; p += 64) {
        uint64_t h;
        uint32_t o;
        if (!kmer_at(L, p, kmask, down, seed, h, o)) continue;
        const uint32_t b = (uint32_t)(h >> bin_shift);
        if (h == L.bins[b] && h != EMPTY) ck::lds_atomic_min(&anchors[b], 2u * (s0 + p) + o);
    }
}

// The starts [s0, s0 + cnt) of the record rec[0 .. n) into L.bins; cnt == 0 or k <= n, s0 + cnt <= n, cnt <= SKETCH_SEG.  Run by
// every lane of a wave, arguments wave-uniform.  Returns the valid k-mers THIS LANE hashed; L.bins is complete in every lane's view.
// With ANCHORS, `anchors` (1 << log2_bins words of LDS) holds the span's anchors afterwards, ANCHOR_NONE where the bin is EMPTY.
template <bool ANCHORS>
CK_DEV uint32_t sketch_span_t(const Sketch& S, const uint8_t* rec, uint32_t n, uint32_t s0, uint32_t cnt, const Lds& L, uint32_t* anchors)
{
    const uint32_t lane = ck::lane_id(), k = S.k, bins = 1u << S.log2_bins;
    for (uint32_t j = lane; j < bins; j += 64) L.bins[j] = EMPTY;
    if (ANCHORS) for (uint32_t j = lane; j < bins; j += 64) anchors[j] = ANCHOR_NONE;
    const uint32_t T = cnt ? cnt + k - 1 : 0, words = (T + 31) / 32;
    if (cnt) pack_span(rec, n, s0, T, words, L);
    ck::wave_sync();
    const uint32_t kmask = k == 32 ? ~0u : (1u << k) - 1u, down = 64 - 2 * k, bin_shift = 64 - S.log2_bins;
    uint32_t valid = 0;
    for (uint32_t p = lane; p < cnt; p += 64) {
        uint64_t h;
        uint32_t o;
        if (!kmer_at(L, p, kmask, down, S.seed, h, o)) continue;
        uint64_t* bin = &L.bins[h >> bin_shift];
        if (h < *bin) lds_min_u64(bin, h);                               // (a bin only decreases: a stale read costs an update, never one)
        ++valid;
    }
    ck::wave_sync();
    if (ANCHORS) {
        anchor_sweep(k, S.log2_bins, S.seed, s0, cnt, L, anchors);
        ck::wave_sync();
    }
    return valid;
}

CK_DEV uint32_t sketch_span(const Sketch& S, const uint8_t* rec, uint32_t n, uint32_t s0, uint32_t cnt, const Lds& L)
{
    return sketch_span_t<false>(S, rec, n, s0, cnt, L, nullptr);
}

// Record `rec` in the short kernel: its row and count when it is one span; an EMPTY row and count 0 otherwise, and the caller is
// told what it is.  *n_valid: its valid k-mers (wave-uniform).
CK_DEV uint32_t short_record(const Sketch& S, uint64_t rec, const Lds& L, uint64_t* n_valid)
{
    const uint32_t lane = ck::lane_id(), bins = 1u << S.log2_bins;
    const uint64_t r0 = S.offsets[rec], len = S.offsets[rec + 1] - r0;   // (offsets that decrease: a length of 2^63 or more, not processed)
    uint64_t* row = S.out + (rec << S.log2_bins);
    *n_valid = 0;
    if (len > SKETCH_SEG) {
        for (uint32_t j = lane; j < bins; j += 64) row[j] = EMPTY;
        if (lane == 0 && S.out_count) S.out_count[rec] = 0;
        return len >= TOO_LONG ? REC_TOO_LONG : REC_LONG;
    }
    const uint32_t n = (uint32_t)len;
    const uint64_t total = ck::wave_sum_u64(sketch_span(S, S.bytes + r0, n, 0, n >= S.k ? n : 0, L));
    for (uint32_t j = lane; j < bins; j += 64) row[j] = L.bins[j];
    if (lane == 0 && S.out_count) S.out_count[rec] = (uint32_t)total;
    ck::wave_sync();                                                     // the bins are read before the next record resets them
    *n_valid = total;
    return REC_DONE;
}

// Workgroup `block` of `grid` of the short kernel: wave w takes records block * SKETCH_WAVES + w, + grid * SKETCH_WAVES, ..
// lds: SKETCH_WAVES * lds_words(log2_bins) 64-bit words, 16-byte aligned.
CK_DEV void short_block(const Sketch& S, uint64_t* lds, uint32_t block, uint32_t grid)
{
    const Lds L = lds_of(lds + (uint64_t)ck::wave_in_block() * lds_words(S.log2_bins));
    uint64_t valid = 0, unprocessed = 0;
    for (uint64_t rec = (uint64_t)block * SKETCH_WAVES + ck::wave_in_block(); rec < S.n_records; rec += (uint64_t)grid * SKETCH_WAVES) {
        uint64_t v;
        const uint32_t kind = short_record(S, rec, L, &v);
        valid += v;
        unprocessed += kind == REC_TOO_LONG;
        if (kind == REC_LONG && ck::lane_id() == 0) S.long_list[global_add_u64(&S.totals[T_LONG], 1)] = rec;
    }
    if (ck::lane_id() == 0) {
        if (valid) global_add_u64(&S.totals[T_VALID], valid);
        if (unprocessed) global_add_u64(&S.totals[T_UNPROCESSED], unprocessed);
    }
}

// Span `seg` of long record `rec`: its bins merged into the record's row, its valid k-mers added to the record's count.  Returns
// them (wave-uniform).
CK_DEV uint64_t long_span(const Sketch& S, uint64_t rec, uint32_t seg, const Lds& L)
{
    const uint32_t lane = ck::lane_id(), bins = 1u << S.log2_bins;
    const uint64_t r0 = S.offsets[rec];
    const uint32_t n = (uint32_t)(S.offsets[rec + 1] - r0);              // SKETCH_SEG < n < 2^31: the short kernel listed it
    const uint32_t s0 = seg * SKETCH_SEG, cnt = n - s0 < SKETCH_SEG ? n - s0 : SKETCH_SEG;
    const uint64_t total = ck::wave_sum_u64(sketch_span(S, S.bytes + r0, n, s0, cnt, L));
    uint64_t* row = S.out + (rec << S.log2_bins);
    for (uint32_t j = lane; j < bins; j += 64) {
        const uint64_t v = L.bins[j];
        if (v != EMPTY) global_min_u64(&row[j], v);
    }
    if (lane == 0 && S.out_count && total) ck::atomic_add_u32(&S.out_count[rec], (uint32_t)total);
    ck::wave_sync();
    return total;
}

// Workgroup `block` of `grid` of the long kernel, over the n_long records of the list.  With as many records as workgroups or more,
// workgroup b takes records b, b + grid, .. and its waves the record's spans in turn; with fewer, grid / n_long workgroups share
// each record's spans, so that one very long record runs on the whole grid.
CK_DEV void long_block(const Sketch& S, uint64_t* lds, uint32_t block, uint32_t grid)
{
    const uint64_t n_long = S.totals[T_LONG];
    if (n_long == 0) return;
    const Lds L = lds_of(lds + (uint64_t)ck::wave_in_block() * lds_words(S.log2_bins));
    uint64_t e = block, e_step = grid;
    uint32_t part = 0, parts = 1;
    if (n_long < grid) {
        parts = grid / (uint32_t)n_long;
        e = block / parts; part = block % parts;
        e_step = n_long;                                                 // one record, or none for the workgroups left over
    }
    uint64_t valid = 0;
    for (; e < n_long; e += e_step) {
        const uint64_t rec = S.long_list[e];
        const uint32_t n = (uint32_t)(S.offsets[rec + 1] - S.offsets[rec]);
        const uint32_t n_seg = (n + SKETCH_SEG - 1) / SKETCH_SEG;
        for (uint32_t seg = part * SKETCH_WAVES + ck::wave_in_block(); seg < n_seg; seg += parts * SKETCH_WAVES) valid += long_span(S, rec, seg, L);
    }
    if (valid && ck::lane_id() == 0) global_add_u64(&S.totals[T_VALID], valid);
}

// ---- anchors ---------------------------------------------------------------------------------------------------------------------
// The "pre-alignment of circular records" section of include/circkit.h: anchor[b] = 2p + o of the smallest start p whose valid
// k-mer has h == row[b], ANCHOR_NONE where row[b] is EMPTY.  The build is the sketch's with one more sweep over the packed starts
// once the bins are final, and an anchor row of 4 bytes a bin in LDS behind the wave's sketch slice.  A long record's row is final
// only behind long_block, so its anchors come from a launch behind that one (anchors_long_block): the spans again, the final row
// read into L.bins, and the 32-bit global minimum of what each span found.  Minimum commutes: the result is the same every run.
struct Anchors {
    Sketch S;
    uint32_t* out_anchor;            // n_records << log2_bins
};

constexpr uint32_t anchors_lds_words(uint32_t log2_bins) { return lds_words(log2_bins) + (1u << log2_bins) / 2; }     // 64-bit words per wave
CK_DEV uint32_t* anchors_of(uint64_t* slice, uint32_t log2_bins) { return (uint32_t*)(slice + lds_words(log2_bins)); }

// short_record with the anchors: a record that is not one span gets a row of ANCHOR_NONE here
CK_DEV uint32_t anchors_short_record(const Anchors& A, uint64_t rec, const Lds& L, uint32_t* anchors, uint64_t* n_valid)
{
    const Sketch& S = A.S;
    const uint32_t lane = ck::lane_id(), bins = 1u << S.log2_bins;
    const uint64_t r0 = S.offsets[rec], len = S.offsets[rec + 1] - r0;
    uint64_t* row = S.out + (rec << S.log2_bins);
    uint32_t* arow = A.out_anchor + (rec << S.log2_bins);
    *n_valid = 0;
    if (len > SKETCH_SEG) {
        for (uint32_t j = lane; j < bins; j += 64) { row[j] = EMPTY; arow[j] = ANCHOR_NONE; }
        if (lane == 0 && S.out_count) S.out_count[rec] = 0;
        return len >= TOO_LONG ? REC_TOO_LONG : REC_LONG;
    }
    const uint32_t n = (uint32_t)len;
    const uint64_t total = ck::wave_sum_u64(sketch_span_t<true>(S, S.bytes + r0, n, 0, n >= S.k ? n : 0, L, anchors));
    for (uint32_t j = lane; j < bins; j += 64) { row[j] = L.bins[j]; arow[j] = anchors[j]; }
    if (lane == 0 && S.out_count) S.out_count[rec] = (uint32_t)total;
    ck::wave_sync();
    *n_valid = total;
    return REC_DONE;
}

// short_block with the anchors.  lds: SKETCH_WAVES * anchors_lds_words(log2_bins) 64-bit words, 16-byte aligned.
CK_DEV void anchors_short_block(const Anchors& A, uint64_t* lds, uint32_t block, uint32_t grid)
{
    const Sketch& S = A.S;
    uint64_t* slice = lds + (uint64_t)ck::wave_in_block() * anchors_lds_words(S.log2_bins);
    const Lds L = lds_of(slice);
    uint32_t* anchors = anchors_of(slice, S.log2_bins);
    uint64_t valid = 0, unprocessed = 0;
    for (uint64_t rec = (uint64_t)block * SKETCH_WAVES + ck::wave_in_block(); rec < S.n_records; rec += (uint64_t)grid * SKETCH_WAVES) {
        uint64_t v;
        const uint32_t kind = anchors_short_record(A, rec, L, anchors, &v);
        valid += v;
        unprocessed += kind == REC_TOO_LONG;
        if (kind == REC_LONG && ck::lane_id() == 0) S.long_list[global_add_u64(&S.totals[T_LONG], 1)] = rec;
    }
    if (ck::lane_id() == 0) {
        if (valid) global_add_u64(&S.totals[T_VALID], valid);
        if (unprocessed) global_add_u64(&S.totals[T_UNPROCESSED], unprocessed);
    }
}

// Span `seg` of long record `rec`, behind long_block: the record's final row into L.bins, the span's anchors into the record's.
CK_DEV void anchors_long_span(const Anchors& A, uint64_t rec, uint32_t seg, const Lds& L, uint32_t* anchors)
{
    const Sketch& S = A.S;
    const uint32_t lane = ck::lane_id(), bins = 1u << S.log2_bins;
    const uint64_t r0 = S.offsets[rec];
    const uint32_t n = (uint32_t)(S.offsets[rec + 1] - r0);              // SKETCH_SEG < n < 2^31: the short kernel listed it
    const uint32_t s0 = seg * SKETCH_SEG, cnt = n - s0 < SKETCH_SEG ? n - s0 : SKETCH_SEG;
    const uint64_t* row = S.out + (rec << S.log2_bins);
    uint32_t* arow = A.out_anchor + (rec << S.log2_bins);
    for (uint32_t j = lane; j < bins; j += 64) { L.bins[j] = row[j]; anchors[j] = ANCHOR_NONE; }
    pack_span(S.bytes + r0, n, s0, cnt + S.k - 1, (cnt + S.k - 1 + 31) / 32, L);
    ck::wave_sync();
    anchor_sweep(S.k, S.log2_bins, S.seed, s0, cnt, L, anchors);
    ck::wave_sync();
    for (uint32_t j = lane; j < bins; j += 64) {
        const uint32_t v = anchors[j];
        if (v != ANCHOR_NONE) global_min_u32(&arow[j], v);
    }
    ck::wave_sync();
}

// long_block's walk over the list, for the anchors; nothing but out_anchor is written
CK_DEV void anchors_long_block(const Anchors& A, uint64_t* lds, uint32_t block, uint32_t grid)
{
    const Sketch& S = A.S;
    const uint64_t n_long = S.totals[T_LONG];
    if (n_long == 0) return;
    uint64_t* slice = lds + (uint64_t)ck::wave_in_block() * anchors_lds_words(S.log2_bins);
    const Lds L = lds_of(slice);
    uint32_t* anchors = anchors_of(slice, S.log2_bins);
    uint64_t e = block, e_step = grid;
    uint32_t part = 0, parts = 1;
    if (n_long < grid) {
        parts = grid / (uint32_t)n_long;
        e = block / parts; part = block % parts;
        e_step = n_long;
    }
    for (; e < n_long; e += e_step) {
        const uint64_t rec = S.long_list[e];
        const uint32_t n = (uint32_t)(S.offsets[rec + 1] - S.offsets[rec]);
        const uint32_t n_seg = (n + SKETCH_SEG - 1) / SKETCH_SEG;
        for (uint32_t seg = part * SKETCH_WAVES + ck::wave_in_block(); seg < n_seg; seg += parts * SKETCH_WAVES) anchors_long_span(A, rec, seg, L, anchors);
    }
}

// ---- the comparison ------------------------------------------------------------------------------------------------------------
struct Compare {
    const uint64_t *a, *b;           // n_a and n_b rows of 1 << log2_bins
    uint64_t n_a, n_b;
    uint32_t log2_bins;
    const uint32_t* pairs;           // (i, j) * n_pairs
    uint64_t n_pairs;
    uint32_t* out;                   // (match, filled) * n_pairs
    uint64_t* n_invalid;
};

// One pair by one wave: a lane takes two bins a step (16 bytes of either row); the counts come from ballots.  Returns whether the
// pair is invalid (wave-uniform): then it is written as (0, 0) and neither row is read.
CK_DEV bool compare_pair(const Compare& C, uint64_t pair)
{
    const uint32_t lane = ck::lane_id(), bins = 1u << C.log2_bins;
    const uint64_t i = C.pairs[2 * pair], j = C.pairs[2 * pair + 1];
    uint32_t match = 0, filled = 0;
    const bool invalid = i >= C.n_a || j >= C.n_b;
    if (!invalid) {
        const uint64_t *ra = C.a + (i << C.log2_bins), *rb = C.b + (j << C.log2_bins);
        for (uint32_t b0 = 0; b0 < bins; b0 += 128) {
            const uint32_t b = b0 + 2 * lane;                            // bins is a multiple of 16: with b, b + 1 is a bin too
            uint64_t x0 = EMPTY, x1 = EMPTY, y0 = EMPTY, y1 = EMPTY;     // a lane past the row: neither a match nor filled
            if (b < bins) {
                const ck::u32x4 x = ck::load16((const uint8_t*)(ra + b)), y = ck::load16((const uint8_t*)(rb + b));
                x0 = ((uint64_t)x.y << 32) | x.x; x1 = ((uint64_t)x.w << 32) | x.z;
                y0 = ((uint64_t)y.y << 32) | y.x; y1 = ((uint64_t)y.w << 32) | y.z;
            }
            match += (uint32_t)ck::popc64(ck::ballot(x0 == y0 && x0 != EMPTY)) + (uint32_t)ck::popc64(ck::ballot(x1 == y1 && x1 != EMPTY));
            filled += (uint32_t)ck::popc64(ck::ballot(x0 != EMPTY || y0 != EMPTY)) + (uint32_t)ck::popc64(ck::ballot(x1 != EMPTY || y1 != EMPTY));
        }
    }
    if (lane == 0) { C.out[2 * pair] = match; C.out[2 * pair + 1] = filled; }
    return invalid;
}

// wave `wave` of `n_waves` takes pairs wave, wave + n_waves, ..
CK_DEV void compare_wave(const Compare& C, uint64_t wave, uint64_t n_waves)
{
    uint64_t bad = 0;
    for (uint64_t p = wave; p < C.n_pairs; p += n_waves) bad += compare_pair(C, p);
    if (bad && ck::lane_id() == 0) global_add_u64(C.n_invalid, bad);
}

}  // namespace ck_sketch
