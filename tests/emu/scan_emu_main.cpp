// CPU fiber run of the shared scan (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that compiles
// circkit_amd/csrc/ck_scan.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber scheduler.  It
// reads a file of cases and writes a file of results (formats: tests/emu/scan_emu.py).  Every routine runs as ONE workgroup of
// WG fibers per run_block, thread tid = 64 * wave_in_block() + lane_id().  The fibers run in their order and each runs until its
// next barrier, so a missing barrier shows only where a LATER fiber then reads what an earlier one has already overwritten (or an
// earlier one reads what a later one has not yet written).  block_scan reads from lower threads only: in ascending order that
// exposes a missing barrier between a step's reads and its writes and a missing last barrier; with --descending, tid = WG - 1 -
// (64 * wave_in_block() + lane_id()), the same fibers expose a missing barrier in front of a step's reads.  A thread that skips a
// barrier deadlocks the workgroup, which the scheduler reports.  The configurations are the product's (WG, ITEMS, Op):
//   0  1024, 8, ck_scan::Add       circkit_orfs.hip
//   1   256, 8, ck_scan::SatAdd    circkit_windows.hip
//   2   256, 2, ck_scan::SatAdd    circkit_fasta_write.hip
//   3   256, 8, PairAdd            circkit_monomerize.hip (restated here: the unit's own lives in the .hip)
//   4   256, 1, StateOp            circkit_fasta.hip's state scan over ck_fasta::next_state (block_scan and the rounds only)
// The LDS array, the sums and the items lie between canaries.
//   scan_emu_main [--descending] CASES RESULTS
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/ck_scan.h"
#include "../../circkit_amd/csrc/fasta_device.h"
#include "../../circkit_amd/csrc/monomer_compact.h"

namespace {

struct Pair { uint64_t cnt, bytes; };                                  // circkit_monomerize.hip's, word for word
inline Pair pair_of(uint64_t w) { return Pair{ w >> 63, w & ~ck_compact::WRITTEN }; }
struct PairAdd {
    typedef Pair T;
    CK_DEV T identity() { return Pair{ 0, 0 }; }
    CK_DEV T combine(T earlier, T later) { return Pair{ earlier.cnt + later.cnt, earlier.bytes + later.bytes }; }
};
struct StateOp {                                                       // circkit_fasta.hip's
    typedef uint32_t T;
    CK_DEV T identity() { return ck_fasta::ST_PASS; }
    CK_DEV T combine(T earlier, T later) { return ck_fasta::next_state(earlier, later); }
};

enum { R_BLOCK_SCAN, R_SUMS_EXCLUSIVE, R_TILE_BASE, R_COMPOSED };
enum { RC_OK = 0, RC_CANARY = 1, RC_THREADS_DISAGREE = 2 };
constexpr size_t GUARD = 8;                                            // elements of canary on either side of an array
constexpr uint8_t CANARY = 0xA5;

bool descending = false;

// an element in the files: W 64-bit words
template <typename T> struct Words { static constexpr int W = 1; static T get(const uint64_t* p) { return (T)p[0]; } static void put(uint64_t* p, T v) { p[0] = v; } };
template <> struct Words<Pair> {
    static constexpr int W = 2;
    static Pair get(const uint64_t* p) { return Pair{ p[0], p[1] }; }
    static void put(uint64_t* p, Pair v) { p[0] = v.cnt; p[1] = v.bytes; }
};
// the element a unit makes of an item's word in memory
template <typename Op> struct Item { static typename Op::T of(uint64_t w) { return (typename Op::T)w; } };
template <> struct Item<PairAdd> { static Pair of(uint64_t w) { return pair_of(w); } };

// n elements between canaries
template <typename T>
struct Guarded {
    std::vector<T> all;
    size_t n;
    explicit Guarded(size_t n_) : all(n_ + 2 * GUARD), n(n_) { memset((void*)all.data(), CANARY, all.size() * sizeof(T)); }
    T* use() { return all.data() + GUARD; }
    bool intact() const
    {
        const uint8_t* b = (const uint8_t*)all.data();
        for (size_t i = 0; i < GUARD * sizeof(T); ++i)
            if (b[i] != CANARY || b[(GUARD + n) * sizeof(T) + i] != CANARY) return false;
        return true;
    }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

template <int WG, int ITEMS, typename Op>
struct Run {
    typedef typename Op::T T;
    static constexpr int W = Words<T>::W;
    static constexpr uint64_t TILE = (uint64_t)WG * ITEMS;

    Guarded<T> lds{ WG };
    uint64_t rc = RC_OK;
    // what the routine at hand reads and writes
    const uint64_t* items = nullptr; uint64_t n = 0, tile = 0;
    T* sums = nullptr; uint64_t n_tiles = 0;
    uint64_t* ends = nullptr;
    std::vector<T> in, out, total;                                     // per thread
    std::vector<uint64_t> loc;                                         // ITEMS words per thread

    Run() : in(WG), out(WG), total(WG), loc(TILE) {}

    static uint32_t tid()
    {
        const uint32_t fiber = 64 * ck::wave_in_block() + ck::lane_id();
        return descending ? WG - 1 - fiber : fiber;
    }
    void launch(void (*body)(void*)) { ck::emu::run_block(body, this, WG / 64); if (!lds.intact()) rc |= RC_CANARY; }
    void all_agree() { for (int t = 1; t < WG; ++t) if (memcmp(&total[t], &total[0], sizeof(T))) rc |= RC_THREADS_DISAGREE; }

    // block_scan, and the LDS array overwritten at once behind it: the last barrier has to be behind the last read
    static void block_scan_body(void* p)
    {
        Run* A = (Run*)p;
        const uint32_t t = tid();
        A->out[t] = ck_scan::block_scan<WG, Op>(t, A->in[t], A->lds.use(), &A->total[t]);
        A->lds.use()[WG - 1 - t] = A->in[t];
    }
    static void tile_sum_body(void* p)
    {
        Run* A = (Run*)p;
        const uint32_t t = tid();
        A->total[t] = ck_scan::tile_sum<WG, ITEMS, Op>(t, A->tile, A->items, A->n, [](uint64_t w) { return Item<Op>::of(w); }, A->lds.use());
        if (t == 0) A->sums[A->tile] = A->total[t];
    }
    static void sums_body(void* p)
    {
        Run* A = (Run*)p;
        const uint32_t t = tid();
        A->total[t] = ck_scan::sums_exclusive<WG, Op>(t, A->sums, A->n_tiles, A->lds.use());
    }
    static void tile_base_body(void* p)
    {
        Run* A = (Run*)p;
        const uint32_t t = tid();
        A->out[t] = ck_scan::tile_base<WG, ITEMS, Op>(t, A->tile, A->items, A->n, [](uint64_t w) { return Item<Op>::of(w); }, A->sums, A->lds.use(),
                                                      &A->loc[(size_t)t * ITEMS]);
    }
    static void apply_body(void* p)
    {
        if constexpr (std::is_same<T, uint64_t>::value) {
            Run* A = (Run*)p;
            ck_scan::apply_ends<WG, ITEMS, Op>(tid(), A->tile, A->ends, A->n, A->sums, A->lds.use());
        }
    }

    void put_elems(FILE* f, const T* v, size_t count)
    {
        std::vector<uint64_t> w(count * W);
        for (size_t k = 0; k < count; ++k) Words<T>::put(&w[k * W], v[k]);
        put(f, w.data(), 8 * w.size());
    }

    // one case: reads what follows its header in the case file, writes its results; 0, or 2 for a case that makes no sense
    int run_case(uint64_t routine, uint64_t n_, uint64_t extra, FILE* in_f, FILE* out_f)
    {
        if (routine == R_BLOCK_SCAN) {
            std::vector<uint64_t> w((size_t)WG * W);
            if (!get(in_f, w.data(), 8 * w.size())) return 2;
            for (int t = 0; t < WG; ++t) in[t] = Words<T>::get(&w[(size_t)t * W]);
            launch(block_scan_body);
            put_elems(out_f, out.data(), WG);
            put_elems(out_f, total.data(), WG);
        } else if (routine == R_SUMS_EXCLUSIVE) {
            std::vector<uint64_t> w(n_ * W);
            if (!get(in_f, w.data(), 8 * w.size())) return 2;
            Guarded<T> s(n_);
            for (uint64_t k = 0; k < n_; ++k) s.use()[k] = Words<T>::get(&w[k * W]);
            sums = s.use(); n_tiles = n_;
            launch(sums_body);
            if (!s.intact()) rc |= RC_CANARY;
            put_elems(out_f, s.use(), n_);
            put_elems(out_f, total.data(), WG);
        } else if (routine == R_TILE_BASE) {
            const uint64_t tiles = (n_ + TILE - 1) / TILE;
            if (extra != tiles) return 2;
            Guarded<uint64_t> it(n_);                                  // (a word read beyond n would be the canary's, not 0)
            std::vector<uint64_t> w(tiles * W);
            if (!get(in_f, it.use(), 8 * n_) || !get(in_f, w.data(), 8 * w.size())) return 2;
            std::vector<T> s(tiles);
            for (uint64_t k = 0; k < tiles; ++k) s[k] = Words<T>::get(&w[k * W]);
            items = it.use(); n = n_; sums = s.data();
            for (tile = 0; tile < tiles; ++tile) {
                launch(tile_base_body);
                put_elems(out_f, out.data(), WG);
                put(out_f, loc.data(), 8 * TILE);
            }
            if (!it.intact()) rc |= RC_CANARY;
        } else if (routine == R_COMPOSED) {
            if constexpr (std::is_same<T, uint64_t>::value) {
                const uint64_t tiles = (n_ + TILE - 1) / TILE;
                Guarded<uint64_t> a(n_), s(tiles);
                if (!get(in_f, a.use(), 8 * n_)) return 2;
                items = a.use(); ends = a.use(); n = n_; sums = s.use(); n_tiles = tiles;
                for (tile = 0; tile < tiles; ++tile) { launch(tile_sum_body); all_agree(); }
                launch(sums_body);
                all_agree();
                const uint64_t grand = total[0];
                for (tile = 0; tile < tiles; ++tile) launch(apply_body);
                if (!a.intact() || !s.intact()) rc |= RC_CANARY;
                put(out_f, a.use(), 8 * n_);
                put(out_f, &grand, 8);
            } else {
                return 2;
            }
        } else {
            return 2;
        }
        put(out_f, &rc, 8);
        return 0;
    }
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "--descending")) { descending = true; ++argv; --argc; }
    if (argc != 3) { fprintf(stderr, "usage: %s [--descending] CASES RESULTS\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t h[4];                                                 // routine, configuration, n, extra
        if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
        int bad = 2;
        if (h[1] == 0) bad = Run<1024, 8, ck_scan::Add>().run_case(h[0], h[2], h[3], in, out);
        else if (h[1] == 1) bad = Run<256, 8, ck_scan::SatAdd>().run_case(h[0], h[2], h[3], in, out);
        else if (h[1] == 2) bad = Run<256, 2, ck_scan::SatAdd>().run_case(h[0], h[2], h[3], in, out);
        else if (h[1] == 3) bad = Run<256, 8, PairAdd>().run_case(h[0], h[2], h[3], in, out);
        else if (h[1] == 4) bad = Run<256, 1, StateOp>().run_case(h[0], h[2], h[3], in, out);
        if (bad) { fprintf(stderr, "case %llu: bad case\n", (unsigned long long)c); return 2; }
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
