// CPU fiber run of the windows gather (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that
// compiles circkit_amd/csrc/window_gather.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler.  It reads a file of cases and writes a file of results (formats: tests/emu/windows_emu.py).  Per case:
// effective_length() runs per window as the lengths kernel's lane runs it; the scan between the two is plain host code with
// the same saturating sum (the scan kernels use no wave routine); gather_tile() runs as a workgroup of the product's
// GATHER_WAVES waves per output tile, so a lane that skips a collective deadlocks its wave, and UBSan + bounds checks watch
// every shift and access.  The payload and the output each lie in an exactly sized heap block between canaries; a lead of a GiB
// and more puts the payload into a lazily reserved mapping instead (tests/emu/lead_block.h).
//   windows_emu_main --constants          prints "TILE_BYTES GATHER_WAVES"
//   windows_emu_main --of-records KIND BASES PERCENT_BITS N...   window_of_record() per length N, as the kernel's lane runs it: one
//                                         line "length record start strand reserved" each (PERCENT_BITS: the f64's bits in hex)
//   windows_emu_main CASES RESULTS
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/window_gather.h"
#include "lead_block.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_LANES_DISAGREE = 1, RC_CANARY = 2 };
enum { REFUSED_CAPACITY = 1 };

struct Launch {
    ck_windows::Gather G;
    uint64_t tile;
    uint64_t first[ck_windows::GATHER_WAVES][64];
};
void body(void* p)
{
    Launch* L = (Launch*)p;
    ck_windows::gather_tile(L->G, L->tile, &L->first[ck::wave_in_block()][ck::lane_id()]);
}

// a block whose byte `shift` past a 64-byte boundary is the first of `size` bytes of use, GUARD canary bytes on either side
struct Block {
    uint8_t* raw = nullptr;
    size_t shift, size;
    uint8_t canary;
    Block(size_t shift_, size_t size_, uint8_t canary_) : shift(shift_), size(size_), canary(canary_)
    {
        if (posix_memalign((void**)&raw, 64, GUARD + shift + size + GUARD)) abort();
        memset(raw, canary, GUARD + shift + size + GUARD);
    }
    ~Block() { free(raw); }
    uint8_t* use() { return raw + GUARD + shift; }
    bool intact(size_t written) const                      // everything but the first `written` bytes of use is still canary
    {
        for (size_t i = 0; i < GUARD + shift; ++i) if (raw[i] != canary) return false;
        for (size_t i = GUARD + shift + written; i < GUARD + shift + size + GUARD; ++i) if (raw[i] != canary) return false;
        return true;
    }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u\n", ck_windows::TILE_BYTES, ck_windows::GATHER_WAVES);
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "--of-records")) {
        const uint32_t kind = (uint32_t)strtoul(argv[2], nullptr, 10);
        const int64_t bases = (int64_t)strtoll(argv[3], nullptr, 10);
        const uint64_t bits = strtoull(argv[4], nullptr, 16);
        double percent;
        memcpy(&percent, &bits, 8);
        for (int i = 5; i < argc; ++i) {
            const ck_windows::Window W = ck_windows::window_of_record(strtoull(argv[i], nullptr, 10), (uint32_t)(i - 5), kind, bases, percent);
            printf("%llu %u %u %u %u\n", (unsigned long long)W.length, W.record, W.start, W.strand, W.reserved);
        }
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULTS | --constants\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    // bio 1.3.1 alphabets::dna complement table, as circkit_ctx_create fills the ctx's
    uint8_t comp[256];
    for (int v = 0; v < 256; ++v) comp[v] = (uint8_t)v;
    const char *x = "AGCTYRWSKMDVHBN", *y = "TCGARYWSMKHBDVN";
    for (int i = 0; x[i]; ++i) { comp[(uint8_t)x[i]] = (uint8_t)y[i]; comp[(uint8_t)x[i] + 32] = (uint8_t)(y[i] + 32); }

    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t h[7];                                     // n_records, n_windows, nb, lead, in_shift, out_shift, capacity (~0: the total)
        if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
        const uint64_t n = h[0], m = h[1], nb = h[2], lead = h[3];
        std::vector<uint64_t> offsets(n + 1), out_offsets(m + 1);
        std::vector<ck_windows::Window> windows(m ? m : 1);
        ck_emu::LeadBlock payload(h[4], lead, nb, IN_CANARY);
        if (!get(in, offsets.data(), 8 * (n + 1)) || !get(in, payload.payload(), nb) || !get(in, windows.data(), sizeof(ck_windows::Window) * m)) {
            fprintf(stderr, "case %llu: short body\n", (unsigned long long)c);
            return 2;
        }
        for (uint64_t& o : offsets) o += lead;
        payload.keep();
        const std::vector<ck_windows::Window> windows_before = windows;

        uint64_t n_invalid = 0, total = 0;
        out_offsets[0] = 0;
        for (uint64_t k = 0; k < m; ++k) {
            bool invalid;
            total = ck_windows::sat_add(total, ck_windows::effective_length(windows[k], offsets.data(), n, &invalid));
            out_offsets[k + 1] = total;
            n_invalid += invalid;
        }
        const uint64_t capacity = h[6] == ~0ull ? total : h[6];
        const uint64_t refused = total > capacity || total == ~0ull ? REFUSED_CAPACITY : 0;
        Block output(h[5], refused ? capacity : total, OUT_CANARY);
        uint64_t rc = RC_OK;
        if (!refused && total && n) {
            Launch L;
            L.G.bytes = payload.use(); L.G.offsets = offsets.data();
            L.G.p0 = offsets[0]; L.G.p1 = offsets[n];
            L.G.windows = windows.data(); L.G.out_offsets = out_offsets.data();
            L.G.m = m; L.G.B = total;
            L.G.comp = comp;
            L.G.out = output.use();
            const uint64_t n_gran = (((uint64_t)(uintptr_t)L.G.out & 15u) + total + 15) / 16;
            const uint64_t n_tiles = (n_gran + ck_windows::TILE_GRANULES - 1) / ck_windows::TILE_GRANULES;
            for (uint64_t t = 0; t < n_tiles && rc == RC_OK; ++t) {
                L.tile = t;
                for (auto& wv : L.first) for (uint64_t& v : wv) v = ~0ull;
                ck::emu::run_block(body, &L, (int)ck_windows::GATHER_WAVES);
                for (auto& wv : L.first)
                    for (int l = 1; l < 64; ++l) if (wv[l] != wv[0]) rc = RC_LANES_DISAGREE;
            }
        }
        const uint64_t written = refused ? 0 : total;
        if (!payload.unchanged() || !output.intact(written) ||
            memcmp(windows_before.data(), windows.data(), sizeof(ck_windows::Window) * m))
            rc = rc ? rc : RC_CANARY;
        const uint64_t r[4] = { rc, total, n_invalid, refused };
        put(out, r, sizeof r);
        put(out, out_offsets.data(), 8 * (m + 1));
        put(out, output.use(), written);
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
