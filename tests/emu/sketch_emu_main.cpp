// CPU fiber run of the sketch unit (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that compiles
// circkit_amd/csrc/sketch.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber scheduler.  It reads
// a file of cases and writes a file of results (formats: tests/emu/sketch_emu.py).  A sketch case runs short_block() as every
// workgroup of the short kernel's grid and then long_block() as every workgroup of the long kernel's, each a workgroup of the
// product's SKETCH_WAVES waves, so a lane that skips a collective deadlocks its wave, and UBSan + bounds checks watch every shift
// and access.  A compare case runs compare_wave() as every wave of its grid.  The payload, the rows, the counts, the list of
// long records, the LDS, the pairs and the results each lie in an exactly sized heap block between canaries, and every input is
// compared with its copy afterwards.
//   sketch_emu_main --constants          prints "SKETCH_SEG SKETCH_WAVES"
//   sketch_emu_main CASES RESULTS
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

#include "../../circkit_amd/csrc/sketch.h"
#include "lead_block.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_CANARY = 2 };
enum { KIND_SKETCH = 0, KIND_COMPARE = 1, KIND_FMIX = 2 };

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
    Block(const Block&) = delete;
    ~Block() { free(raw); }
    uint8_t* use() { return raw + GUARD + shift; }
    bool intact() const                                    // the guards on either side are still canary
    {
        for (size_t i = 0; i < GUARD + shift; ++i) if (raw[i] != canary) return false;
        for (size_t i = GUARD + shift + size; i < GUARD + shift + size + GUARD; ++i) if (raw[i] != canary) return false;
        return true;
    }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
bool changed(const std::vector<uint8_t>& before, const uint8_t* now) { return !before.empty() && memcmp(before.data(), now, before.size()) != 0; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

struct SketchLaunch {
    ck_sketch::Sketch S;
    uint64_t* lds;
    uint32_t block, grid;
};
void short_body(void* p) { SketchLaunch* L = (SketchLaunch*)p; ck_sketch::short_block(L->S, L->lds, L->block, L->grid); }
void long_body(void* p) { SketchLaunch* L = (SketchLaunch*)p; ck_sketch::long_block(L->S, L->lds, L->block, L->grid); }

struct CompareLaunch {
    ck_sketch::Compare C;
    uint64_t wave, n_waves;
};
void compare_body(void* p) { CompareLaunch* L = (CompareLaunch*)p; ck_sketch::compare_wave(L->C, L->wave, L->n_waves); }

int sketch_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[10];    // n_records, payload bytes, lead, in_shift, k, log2_bins, seed, short grid, long grid, want_counts
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0], nb = h[1], lead = h[2], bins = 1ull << h[5];
    std::vector<uint64_t> offsets(n + 1);
    ck_emu::LeadBlock payload(h[3], lead, nb, IN_CANARY);
    if (!get(in, offsets.data(), 8 * (n + 1)) || !get(in, payload.payload(), nb)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
    for (uint64_t& o : offsets) o += lead;
    payload.keep();
    const std::vector<uint64_t> offsets_before = offsets;

    Block rows(0, n * bins * 8, OUT_CANARY), counts(0, n * 4, OUT_CANARY), list(0, n * 8, OUT_CANARY);
    Block lds(0, (size_t)ck_sketch::SKETCH_WAVES * ck_sketch::lds_words((uint32_t)h[5]) * 8, OUT_CANARY);
    uint64_t totals[ck_sketch::T_WORDS] = { 0, 0, 0 };
    SketchLaunch L;
    L.S.bytes = payload.use(); L.S.offsets = offsets.data(); L.S.n_records = n;
    L.S.k = (uint32_t)h[4]; L.S.log2_bins = (uint32_t)h[5]; L.S.seed = h[6];
    L.S.out = (uint64_t*)rows.use(); L.S.out_count = h[9] ? (uint32_t*)counts.use() : nullptr;
    L.S.long_list = (uint64_t*)list.use(); L.S.totals = totals;
    L.lds = (uint64_t*)lds.use();
    if (n) {
        L.grid = (uint32_t)h[7];
        for (L.block = 0; L.block < L.grid; ++L.block) ck::emu::run_block(short_body, &L, (int)ck_sketch::SKETCH_WAVES);
        L.grid = (uint32_t)h[8];
        for (L.block = 0; L.block < L.grid; ++L.block) ck::emu::run_block(long_body, &L, (int)ck_sketch::SKETCH_WAVES);
    }
    uint64_t rc = RC_OK;
    if (!payload.unchanged() || offsets != offsets_before || !rows.intact() || !counts.intact() ||
        !list.intact() || !lds.intact())
        rc = RC_CANARY;
    if (!h[9]) for (size_t i = 0; i < n * 4; ++i) if (counts.use()[i] != OUT_CANARY) rc = RC_CANARY;
    const uint64_t r[4] = { rc, totals[ck_sketch::T_VALID], totals[ck_sketch::T_UNPROCESSED], totals[ck_sketch::T_LONG] };
    put(out, r, sizeof r);
    put(out, rows.use(), n * bins * 8);
    if (h[9]) put(out, counts.use(), n * 4);
    return 0;
}

int compare_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[6];     // n_a, n_b, log2_bins, n_pairs, same, n_waves
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n_a = h[0], n_b = h[1], bins = 1ull << h[2], m = h[3];
    const bool same = h[4] != 0;
    Block a(0, n_a * bins * 8, IN_CANARY), b(8, same ? 0 : n_b * bins * 8, IN_CANARY), pairs(0, m * 8, IN_CANARY), res(0, m * 8, OUT_CANARY);
    if (!get(in, a.use(), a.size) || !get(in, b.use(), b.size) || !get(in, pairs.use(), pairs.size)) {
        fprintf(stderr, "case %llu: short body\n", (unsigned long long)c);
        return 2;
    }
    const std::vector<uint8_t> a0(a.use(), a.use() + a.size), b0(b.use(), b.use() + b.size), p0(pairs.use(), pairs.use() + pairs.size);
    uint64_t n_invalid = 0;
    CompareLaunch L;
    L.C.a = (const uint64_t*)a.use(); L.C.b = same ? L.C.a : (const uint64_t*)b.use();
    L.C.n_a = n_a; L.C.n_b = n_b; L.C.log2_bins = (uint32_t)h[2];
    L.C.pairs = (const uint32_t*)pairs.use(); L.C.n_pairs = m;
    L.C.out = (uint32_t*)res.use(); L.C.n_invalid = &n_invalid;
    L.n_waves = h[5];
    for (L.wave = 0; m && L.wave < L.n_waves; ++L.wave) ck::emu::run_block(compare_body, &L, 1);
    uint64_t rc = RC_OK;
    if (!a.intact() || !b.intact() || !pairs.intact() || !res.intact() || changed(a0, a.use()) || changed(b0, b.use()) || changed(p0, pairs.use()))
        rc = RC_CANARY;
    const uint64_t r[2] = { rc, n_invalid };
    put(out, r, sizeof r);
    put(out, res.use(), m * 8);
    return 0;
}

int fmix_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t n;
    if (!get(in, &n, 8)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    std::vector<uint64_t> w(n);
    if (!get(in, w.data(), 8 * n)) return 2;
    for (uint64_t& v : w) v = ck_sketch::fmix64(v);
    put(out, w.data(), 8 * n);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u\n", ck_sketch::SKETCH_SEG, ck_sketch::SKETCH_WAVES);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULTS | --constants\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t kind;
        if (!get(in, &kind, 8)) { fprintf(stderr, "case %llu: no kind\n", (unsigned long long)c); return 2; }
        const int rc = kind == KIND_SKETCH ? sketch_case(in, out, c) : kind == KIND_COMPARE ? compare_case(in, out, c) : fmix_case(in, out, c);
        if (rc) return rc;
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
