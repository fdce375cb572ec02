// CPU fiber run of the distance unit (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that compiles
// circkit_amd/csrc/distance.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber scheduler.  It
// reads a file of cases and writes a file of results (formats: tests/emu/distance_emu.py).  A case runs pairs_wave() as every wave
// of its grid, each wave with a slice of LDS of the product's size.  A lane that skips a collective deadlocks its wave, and UBSan +
// bounds checks watch every shift and access.  The payloads, the offsets, the pairs, the LDS slice, the distances and the scores
// each lie in an exactly sized heap block between canaries, and every input is compared with its copy afterwards.
//   distance_emu_main --constants          prints "DISTANCE_WAVES SLICE_WORDS STAGE_SLACK DISTANCE_MAX"
//   distance_emu_main CASES RESULTS
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

#include "../../circkit_amd/csrc/distance.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_CANARY = 2 };

// `size` bytes of use at a 64-byte boundary, GUARD canary bytes on either side
struct Block {
    uint8_t* raw = nullptr;
    size_t size;
    uint8_t canary;
    Block(size_t size_, uint8_t canary_) : size(size_), canary(canary_)
    {
        if (posix_memalign((void**)&raw, 64, GUARD + size + GUARD)) abort();
        memset(raw, canary, GUARD + size + GUARD);
    }
    Block(const Block&) = delete;
    ~Block() { free(raw); }
    uint8_t* use() { return raw + GUARD; }
    bool intact() const
    {
        for (size_t i = 0; i < GUARD; ++i) if (raw[i] != canary || raw[GUARD + size + i] != canary) return false;
        return true;
    }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }
bool changed(const std::vector<uint8_t>& before, const uint8_t* now) { return !before.empty() && memcmp(before.data(), now, before.size()) != 0; }

struct PairsLaunch { ck_distance::Distance D; uint32_t* slice; uint64_t wave, n_waves; };
void pairs_body(void* p) { PairsLaunch* L = (PairsLaunch*)p; ck_distance::pairs_wave(L->D, L->slice, L->wave, L->n_waves); }

int one_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[9];     // n_a, payload bytes of A, n_b, payload bytes of B, same batch, W, n_pairs, outputs (1 distance | 2 scores), waves
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n_a = h[0], nb_a = h[1], same = h[4], n_b = same ? n_a : h[2], nb_b = same ? 0 : h[3], m = h[6];
    Block off_a((n_a + 1) * 8, IN_CANARY), pay_a(nb_a, IN_CANARY), off_b(same ? 0 : (n_b + 1) * 8, IN_CANARY), pay_b(nb_b, IN_CANARY), pairs(m * 8, IN_CANARY);
    if (!get(in, off_a.use(), off_a.size) || !get(in, pay_a.use(), nb_a) || !get(in, off_b.use(), off_b.size) || !get(in, pay_b.use(), nb_b) ||
        !get(in, pairs.use(), pairs.size)) {
        fprintf(stderr, "case %llu: short body\n", (unsigned long long)c);
        return 2;
    }
    const std::vector<uint8_t> oa0(off_a.use(), off_a.use() + off_a.size), pa0(pay_a.use(), pay_a.use() + nb_a), ob0(off_b.use(), off_b.use() + off_b.size),
        pb0(pay_b.use(), pay_b.use() + nb_b), p0(pairs.use(), pairs.use() + pairs.size);
    Block dist(m * 4, OUT_CANARY), scores(m * 8, OUT_CANARY), slice((size_t)ck_distance::SLICE_WORDS * 4, OUT_CANARY);
    uint64_t totals[ck_distance::T_WORDS] = { 0, 0 };
    PairsLaunch L;
    L.D.bytes_a = pay_a.use(); L.D.offsets_a = (const uint64_t*)off_a.use(); L.D.n_a = n_a;
    L.D.bytes_b = same ? pay_a.use() : pay_b.use(); L.D.offsets_b = (const uint64_t*)(same ? off_a.use() : off_b.use()); L.D.n_b = n_b;
    L.D.max_distance = (uint32_t)h[5];
    L.D.pairs = (const uint32_t*)pairs.use(); L.D.n_pairs = m;
    L.D.distance = (h[7] & 1) ? (uint32_t*)dist.use() : nullptr;
    L.D.scores = (h[7] & 2) ? (uint32_t*)scores.use() : nullptr;
    L.D.totals = totals;
    L.slice = (uint32_t*)slice.use();
    L.n_waves = h[8];
    for (L.wave = 0; m && L.wave < L.n_waves; ++L.wave) ck::emu::run_block(pairs_body, &L, 1);
    uint64_t rc = RC_OK;
    if (!off_a.intact() || !pay_a.intact() || !off_b.intact() || !pay_b.intact() || !pairs.intact() || !dist.intact() || !scores.intact() ||
        !slice.intact() || changed(oa0, off_a.use()) || changed(pa0, pay_a.use()) || changed(ob0, off_b.use()) || changed(pb0, pay_b.use()) ||
        changed(p0, pairs.use()))
        rc = RC_CANARY;
    const uint64_t r[3] = { rc, totals[ck_distance::T_WITHIN], totals[ck_distance::T_INVALID] };
    put(out, r, sizeof r);
    put(out, dist.use(), dist.size);
    put(out, scores.use(), scores.size);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u %u %u\n", ck_distance::DISTANCE_WAVES, ck_distance::SLICE_WORDS, ck_distance::STAGE_SLACK, ck_distance::DISTANCE_MAX);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULTS | --constants\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        const int rc = one_case(in, out, c);
        if (rc) return rc;
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
