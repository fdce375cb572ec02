// orfs.h -- circular ORF finding for one record (the reference's src/orfs.rs worker closure = lib/src/orfs.rs
// start_stop_codon_indices_by_frame_naive + find_orfs_with_indices + the CLI filter + longest_orfs), written as ONE
// streaming pass per strand that needs no per-record lists: orf_strand() below runs on one lane.
//
// Symbols are coded in 3 bits (A C G T N - = 0..5, any other byte 6), a codon in 9 bits, and a 512-entry class table says
// whether a codon is in the start set (bit 0) and in the stop set (bit 1).  A set codon holding a byte outside {ACGTN-}
// never enters the table: records are normalized, so it could never match.  The reverse strand is read from the same
// forward bytes: its symbol j is complement(fwd[L - 1 - j]), and the complement of a code is 3 - code for A C G T and the
// code itself otherwise (bio's table maps N, '-' and every other normalized byte to a byte of the same class).
//
// Classification (lib/src/orfs.rs:83-91): positions 0..L-3 are start, or failing that stop, never both; the two wrapping
// codons at L-2 and L-1 are tested against each set separately (add_last_codons, :57-70).
//
// Next stop of a start p in frame f = p % 3 (:149-298).  The sweep runs from position L-1 down to 0 and carries, per frame,
// the nearest stop at or after the current position (L % 3 != 0: `>= start`) or strictly after it (L % 3 == 0: `> start`;
// a codon that is both is taken as a start before it is taken as a stop).  A start with no such stop wraps:
//  - L % 3 == 0: the first stop of its own frame if that is before it, else None (length L, wraps 1);
//  - otherwise the first stop of frame (f - L) mod 3, then the next frame, then f again (laps 1, 2, 3), else None
//    (length 3L, wraps 3).  first_stop[3] comes from a short forward prologue that stops once every frame has one.
// With t = the unrolled distance from the start's lap origin to the stop, wraps = floor((t + 2) / L) in every case.
//
// Longest per stop (:301-315) without sets or sorting by stop: the starts sharing a stop form a contiguous stretch of the
// reading-frame chain that ends at that stop; along it, lengths fall and wraps do not rise, so every filter passes a
// prefix of it except max_wraps, which passes a suffix.  The ORF kept for a stop is therefore the first start of its
// stretch (in chain order) that passes, and a start r is kept iff it passes and its chain predecessor q in the stretch
// (if any) fails -- q only fails max_wraps, and wraps(q) = wraps(r) + k where k = the origin crossings between them.
// Going backwards, each frame holds one pending start and decides it when the sweep meets the next start of the frame (k =
// 0: not kept), a stop (no q: kept iff it passes), or the beginning of the record (q is found from the last event of the
// frame(s) before, in chain order: k laps back).  The None key is one group across frames: every member has the same
// length and wraps, and longest_orfs keeps the one that comes last in find order (highest frame, then highest start).
//
// The emitted ORFs of a strand are in no particular order; the caller sorts them (sort_run).
#pragma once
#include <stdint.h>

namespace ck_orfs {

constexpr uint32_t NO_STOP = 0xFFFFFFFFu;
constexpr uint32_t CLS_START = 1, CLS_STOP = 2;

struct Orf {               // = circkit_orf
    uint64_t length;
    uint32_t start, stop, wraps, strand;
};

struct Filter {
    uint64_t min_length;
    double min_ratio;
    uint32_t min_wraps, max_wraps, require_stop, mode;   // mode 0 = longest per stop, 1 = every ORF
};

__host__ __device__ inline uint32_t sym_code(uint8_t b)
{
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : b == 'N' ? 4u : b == '-' ? 5u : 6u;
}
__host__ __device__ inline uint32_t comp_code(uint32_t c) { return c < 4 ? 3 - c : c; }

__device__ inline bool passes(const Filter& F, uint64_t length, uint32_t stop, uint32_t wraps, uint64_t L)
{
    // src/orfs.rs:68-74: the ratio is an f64 division (correctly rounded: no fast-math in this build)
    return length - 3 >= F.min_length && (!F.require_stop || stop != NO_STOP) && F.min_wraps <= wraps &&
           wraps <= F.max_wraps && (double)length / (double)L >= F.min_ratio;
}

// the order of longest_orfs' output (stable ascending sort by length, reversed): length, then frame, then start, all
// descending; mode 1 = find order (frame-major, start ascending)
__host__ __device__ inline bool orf_before(const Orf& a, const Orf& b, uint32_t mode)
{
    const uint32_t fa = a.start % 3, fb = b.start % 3;
    if (mode == 1) return fa != fb ? fa < fb : a.start < b.start;
    if (a.length != b.length) return a.length > b.length;
    return fa != fb ? fa > fb : a.start > b.start;
}

constexpr uint32_t SORT_INSERTION_MAX = 32;   // runs up to this many ORFs sort by insertion, longer ones by heapsort

// Sorts one strand's run of a record into orf_before's order, in place and without scratch memory (one lane of the emit
// kernel; the host build of the lane routine calls it too).
__host__ __device__ inline void sort_run(Orf* a, uint32_t n, uint32_t mode)
{
    if (n <= SORT_INSERTION_MAX) {
        for (uint32_t i = 1; i < n; ++i) {
            const Orf x = a[i];
            uint32_t j = i;
            for (; j > 0 && orf_before(x, a[j - 1], mode); --j) a[j] = a[j - 1];
            a[j] = x;
        }
        return;
    }
    // heapsort, a max-heap under orf_before's reverse (the root is the element that goes last)
    auto sift = [&](uint32_t root, uint32_t end) {
        const Orf x = a[root];
        for (;;) {
            uint32_t child = 2 * root + 1;
            if (child >= end) break;
            if (child + 1 < end && orf_before(a[child], a[child + 1], mode)) ++child;
            if (!orf_before(x, a[child], mode)) break;
            a[root] = a[child];
            root = child;
        }
        a[root] = x;
    };
    for (uint32_t r = n / 2; r-- > 0;) sift(r, n);
    for (uint32_t end = n - 1; end > 0; --end) {
        const Orf t = a[0]; a[0] = a[end]; a[end] = t;
        sift(0, end);
    }
}

// symbol j of the strand (REV: the reverse complement of the record)
template <bool REV>
__device__ inline uint32_t strand_sym(const uint8_t* __restrict__ s, uint32_t L, uint32_t j)
{
    return REV ? comp_code(sym_code(s[L - 1 - j])) : sym_code(s[j]);
}

// One strand of one record (2 <= L < 2^32).  emit(const Orf&) is called for every ORF the reference would output for this
// strand; returns how many.  cls: the 512-entry class table.
template <bool REV, typename Emit>
__device__ uint32_t orf_strand(const uint8_t* __restrict__ s, uint32_t L, const uint8_t* cls, const Filter& F, uint32_t strand,
                               Emit&& emit)
{
    const uint32_t Lm3 = L % 3;
    const uint64_t L64 = L;
    auto classify = [&](uint32_t j, uint32_t codon) -> uint32_t {
        uint32_t c = cls[codon];
        if (j + 2 < L && (c & CLS_START)) c = CLS_START;         // interior: start, else stop (never both)
        return c;
    };
    // ---- prologue: the first stop of each frame (forward, until all three are known) ----
    uint32_t first_stop[3] = { NO_STOP, NO_STOP, NO_STOP };
    {
        uint32_t codon = (strand_sym<REV>(s, L, 0) << 6) | (strand_sym<REV>(s, L, 1) << 3) | strand_sym<REV>(s, L, 2 % L);
        uint32_t f = 0, found = 0;
        for (uint32_t j = 0; j < L && found < 3; ++j) {
            if (j) codon = ((codon << 3) | strand_sym<REV>(s, L, (uint32_t)((j + 2ull) % L))) & 511u;
            if ((classify(j, codon) & CLS_STOP) && first_stop[f] == NO_STOP) { first_stop[f] = j; ++found; }
            f = f == 2 ? 0 : f + 1;
        }
    }
    // ---- backward sweep ----
    uint32_t carry[3] = { NO_STOP, NO_STOP, NO_STOP };           // nearest stop after the position, per frame
    uint32_t n_stops[3] = { 0, 0, 0 };
    uint32_t last_ev[3] = { 0, 0, 0 };                           // class of the frame's last event (0 = none yet)
    Orf pending[3];
    bool has_pending[3] = { false, false, false };
    bool has_none = false;
    Orf none_best;
    uint32_t count = 0;

    auto orf_of = [&](uint32_t p, uint32_t f) -> Orf {
        Orf o; o.start = p; o.strand = strand;
        if (carry[f] != NO_STOP) {
            const uint32_t st = carry[f];
            o.stop = st; o.length = (uint64_t)(st - p) + 3; o.wraps = L - st < 3 ? 1 : 0;
            return o;
        }
        if (Lm3 == 0) {
            const uint32_t st = first_stop[f];
            if (st != NO_STOP && st < p) { o.stop = st; o.length = (uint64_t)st + L64 - p + 3; o.wraps = 1; }
            else { o.stop = NO_STOP; o.length = L64; o.wraps = 1; }
            return o;
        }
        uint64_t len = L64 - p;
        uint32_t cur = f;
        for (uint32_t lap = 1; lap <= 3; ++lap) {
            cur = Lm3 == 2 ? (cur == 2 ? 0 : cur + 1) : (cur == 0 ? 2 : cur - 1);
            const uint32_t st = first_stop[cur];
            if (st != NO_STOP) {
                o.stop = st; o.length = len + st + 3;
                o.wraps = lap == 3 ? 3 : (L - st >= 3 ? lap : lap + 1);
                return o;
            }
            len += lap < 3 ? L64 : (uint64_t)p;
        }
        o.stop = NO_STOP; o.length = len; o.wraps = 3;
        return o;
    };
    auto take = [&](const Orf& o) { emit(o); ++count; };
    auto on_stop = [&](uint32_t j, uint32_t f, uint32_t c) {
        if (!last_ev[f]) last_ev[f] = c;
        ++n_stops[f];
        if (has_pending[f]) {                                    // the stretch of the stop before starts here: no q
            if (passes(F, pending[f].length, pending[f].stop, pending[f].wraps, L64)) take(pending[f]);
            has_pending[f] = false;
        }
        carry[f] = j;
    };
    auto on_start = [&](uint32_t j, uint32_t f, uint32_t c) {
        if (!last_ev[f]) last_ev[f] = c;
        const Orf o = orf_of(j, f);
        if (F.mode == 1) { if (passes(F, o.length, o.stop, o.wraps, L64)) take(o); return; }
        if (o.stop == NO_STOP) {
            // same length and wraps for every member; the sweep meets frames' starts in descending order
            if (passes(F, o.length, o.stop, o.wraps, L64) &&
                (!has_none || f > none_best.start % 3 || (f == none_best.start % 3 && j > none_best.start))) {
                none_best = o; has_none = true;
            }
            return;
        }
        has_pending[f] = true;                                   // a pending start of this stretch (k = 0) is not kept
        pending[f] = o;
    };

    {
        uint32_t codon = (strand_sym<REV>(s, L, L - 1) << 6) | (strand_sym<REV>(s, L, 0) << 3) | strand_sym<REV>(s, L, 1 % L);
        uint32_t f = (L - 1) % 3;
        for (uint32_t j = L; j-- > 0;) {
            if (j != L - 1) codon = (strand_sym<REV>(s, L, j) << 6) | (codon >> 3);
            const uint32_t c = classify(j, codon);
            if (c) {
                if (Lm3 == 0) {                                  // `> start`: the start belongs to the stretch after it
                    if (c & CLS_START) on_start(j, f, c);
                    if (c & CLS_STOP) on_stop(j, f, c);
                } else {                                         // `>= start`: a codon that is both is its own stop
                    if (c & CLS_STOP) on_stop(j, f, c);
                    if (c & CLS_START) on_start(j, f, c);
                }
            }
            f = f == 0 ? 2 : f - 1;
        }
    }
    // ---- the first stretch of each frame: its chain predecessor lies k laps back ----
    for (uint32_t f = 0; f < 3; ++f) {
        if (!has_pending[f]) continue;
        const Orf& r = pending[f];
        bool q = false;
        uint32_t k = 1;
        if (Lm3 == 0) {
            // the frame's last event: a start, or a codon that is both when it is not the frame's only stop
            q = last_ev[f] == CLS_START || (last_ev[f] == (CLS_START | CLS_STOP) && n_stops[f] >= 2);
        } else {
            uint32_t g = f;
            for (; k <= 3; ++k) {
                g = (g + Lm3) % 3;                               // the frame whose lap ends where f begins
                if (!last_ev[g]) continue;
                q = last_ev[g] == CLS_START;                     // a stop (or a codon that is both) ends the stretch
                break;
            }
        }
        if (passes(F, r.length, r.stop, r.wraps, L64) && !(q && r.wraps + k <= F.max_wraps)) take(r);
    }
    if (has_none) take(none_best);
    return count;
}

}  // namespace ck_orfs
