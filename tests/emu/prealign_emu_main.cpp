// CPU fiber run of the prealign unit and of the anchor routines of the sketch unit (TEST INFRASTRUCTURE ONLY, never linked into the
// product): a stand-alone program that compiles circkit_amd/csrc/prealign.h and sketch.h against tests/emu/wave_prims_emu.h and
// links against libcanon_emu.so for the fiber scheduler.  It reads a file of cases and writes a file of results (formats:
// tests/emu/prealign_emu.py).  An anchors case runs anchors_short_block() as every workgroup of the short kernel's grid, then
// long_block() and anchors_long_block() as every workgroup of the long kernels', each a workgroup of the product's SKETCH_WAVES
// waves; a votes case runs pairs_wave() as every wave of its grid, a labels case labels_lane() as every lane of its grid.  A lane
// that skips a collective deadlocks its wave, and UBSan + bounds checks watch every shift and access.  The payload, the rows, the
// counts, the anchors, the list of long records, the LDS, the pairs, the windows and the scores each lie in an exactly sized heap
// block between canaries, and every input is compared with its copy afterwards.
//   prealign_emu_main --constants          prints "SKETCH_SEG SKETCH_WAVES PREALIGN_WAVES"
//   prealign_emu_main CASES RESULTS
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

#include "../../circkit_amd/csrc/prealign.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_CANARY = 2 };
enum { KIND_ANCHORS = 0, KIND_VOTES = 1, KIND_LABELS = 2 };

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

struct AnchorsLaunch { ck_sketch::Anchors A; uint64_t* lds; uint32_t block, grid; };
void short_body(void* p) { AnchorsLaunch* L = (AnchorsLaunch*)p; ck_sketch::anchors_short_block(L->A, L->lds, L->block, L->grid); }
void long_body(void* p) { AnchorsLaunch* L = (AnchorsLaunch*)p; ck_sketch::long_block(L->A.S, L->lds, L->block, L->grid); }
void anchors_long_body(void* p) { AnchorsLaunch* L = (AnchorsLaunch*)p; ck_sketch::anchors_long_block(L->A, L->lds, L->block, L->grid); }

struct PairsLaunch { ck_prealign::Prealign P; uint32_t* keys; uint64_t wave, n_waves; };
void pairs_body(void* p) { PairsLaunch* L = (PairsLaunch*)p; ck_prealign::pairs_wave(L->P, L->keys, L->wave, L->n_waves); }

struct LabelsLaunch { const uint64_t* labels; uint64_t n; uint32_t* pairs; uint64_t wave, n_waves; };
void labels_body(void* p)
{
    LabelsLaunch* L = (LabelsLaunch*)p;
    ck_prealign::labels_lane(L->labels, L->n, L->pairs, L->wave * 64 + ck::lane_id(), L->n_waves * 64);
}

int anchors_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[9];     // n_records, payload bytes, lead, k, log2_bins, seed, short grid, long grid, want_counts
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0], nb = h[1], lead = h[2], bins = 1ull << h[4];
    std::vector<uint64_t> offsets(n + 1);
    Block payload(lead + nb, IN_CANARY);
    if (!get(in, offsets.data(), 8 * (n + 1)) || !get(in, payload.use() + lead, nb)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
    for (uint64_t& o : offsets) o += lead;
    const std::vector<uint8_t> before(payload.use(), payload.use() + lead + nb);
    const std::vector<uint64_t> offsets_before = offsets;

    Block rows(n * bins * 8, OUT_CANARY), counts(n * 4, OUT_CANARY), anchors(n * bins * 4, OUT_CANARY), list(n * 8, OUT_CANARY);
    Block lds((size_t)ck_sketch::SKETCH_WAVES * ck_sketch::anchors_lds_words((uint32_t)h[4]) * 8, OUT_CANARY);
    uint64_t totals[ck_sketch::T_WORDS] = { 0, 0, 0 };
    AnchorsLaunch L;
    ck_sketch::Sketch& S = L.A.S;
    S.bytes = payload.use(); S.offsets = offsets.data(); S.n_records = n;
    S.k = (uint32_t)h[3]; S.log2_bins = (uint32_t)h[4]; S.seed = h[5];
    S.out = (uint64_t*)rows.use(); S.out_count = h[8] ? (uint32_t*)counts.use() : nullptr;
    S.long_list = (uint64_t*)list.use(); S.totals = totals;
    L.A.out_anchor = (uint32_t*)anchors.use();
    L.lds = (uint64_t*)lds.use();
    if (n) {
        L.grid = (uint32_t)h[6];
        for (L.block = 0; L.block < L.grid; ++L.block) ck::emu::run_block(short_body, &L, (int)ck_sketch::SKETCH_WAVES);
        L.grid = (uint32_t)h[7];
        for (L.block = 0; L.block < L.grid; ++L.block) ck::emu::run_block(long_body, &L, (int)ck_sketch::SKETCH_WAVES);
        for (L.block = 0; L.block < L.grid; ++L.block) ck::emu::run_block(anchors_long_body, &L, (int)ck_sketch::SKETCH_WAVES);
    }
    uint64_t rc = RC_OK;
    if (!payload.intact() || changed(before, payload.use()) || offsets != offsets_before || !rows.intact() || !counts.intact() ||
        !anchors.intact() || !list.intact() || !lds.intact())
        rc = RC_CANARY;
    if (!h[8]) for (size_t i = 0; i < n * 4; ++i) if (counts.use()[i] != OUT_CANARY) rc = RC_CANARY;
    const uint64_t r[4] = { rc, totals[ck_sketch::T_VALID], totals[ck_sketch::T_UNPROCESSED], totals[ck_sketch::T_LONG] };
    put(out, r, sizeof r);
    put(out, rows.use(), rows.size);
    put(out, anchors.use(), anchors.size);
    if (h[8]) put(out, counts.use(), counts.size);
    return 0;
}

int votes_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[6];     // n_records, log2_bins, k, min_votes, n_pairs, n_waves
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0], bins = 1ull << h[1], m = h[4];
    Block rows(n * bins * 8, IN_CANARY), anchors(n * bins * 4, IN_CANARY), offsets((n + 1) * 8, IN_CANARY), pairs(m * 8, IN_CANARY);
    Block windows(m * ck_prealign::WINDOW_BYTES, OUT_CANARY), scores(m * 8, OUT_CANARY), keys(bins * 4, OUT_CANARY);
    if (!get(in, rows.use(), rows.size) || !get(in, anchors.use(), anchors.size) || !get(in, offsets.use(), offsets.size) ||
        !get(in, pairs.use(), pairs.size)) {
        fprintf(stderr, "case %llu: short body\n", (unsigned long long)c);
        return 2;
    }
    const std::vector<uint8_t> r0(rows.use(), rows.use() + rows.size), a0(anchors.use(), anchors.use() + anchors.size),
        o0(offsets.use(), offsets.use() + offsets.size), p0(pairs.use(), pairs.use() + pairs.size);
    uint64_t totals[ck_prealign::T_WORDS] = { 0, 0 };
    PairsLaunch L;
    L.P.rows = (const uint64_t*)rows.use(); L.P.anchors = (const uint32_t*)anchors.use(); L.P.offsets = (const uint64_t*)offsets.use();
    L.P.n_records = n; L.P.k = (uint32_t)h[2]; L.P.log2_bins = (uint32_t)h[1]; L.P.min_votes = (uint32_t)h[3];
    L.P.pairs = (const uint32_t*)pairs.use(); L.P.n_pairs = m;
    L.P.windows = windows.use(); L.P.scores = (uint32_t*)scores.use(); L.P.totals = totals;
    L.keys = (uint32_t*)keys.use();
    L.n_waves = h[5];
    for (L.wave = 0; m && L.wave < L.n_waves; ++L.wave) ck::emu::run_block(pairs_body, &L, 1);
    uint64_t rc = RC_OK;
    if (!rows.intact() || !anchors.intact() || !offsets.intact() || !pairs.intact() || !windows.intact() || !scores.intact() || !keys.intact() ||
        changed(r0, rows.use()) || changed(a0, anchors.use()) || changed(o0, offsets.use()) || changed(p0, pairs.use()))
        rc = RC_CANARY;
    const uint64_t r[3] = { rc, totals[ck_prealign::T_ALIGNED], totals[ck_prealign::T_INVALID] };
    put(out, r, sizeof r);
    put(out, windows.use(), windows.size);
    put(out, scores.use(), scores.size);
    return 0;
}

int labels_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[2];     // n_records, n_waves
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0];
    Block labels(n * 8, IN_CANARY), pairs(n * 8, OUT_CANARY);
    if (!get(in, labels.use(), labels.size)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
    const std::vector<uint8_t> l0(labels.use(), labels.use() + labels.size);
    LabelsLaunch L;
    L.labels = (const uint64_t*)labels.use(); L.n = n; L.pairs = (uint32_t*)pairs.use();
    L.n_waves = h[1];
    for (L.wave = 0; n && L.wave < L.n_waves; ++L.wave) ck::emu::run_block(labels_body, &L, 1);
    const uint64_t rc = !labels.intact() || !pairs.intact() || changed(l0, labels.use()) ? RC_CANARY : RC_OK;
    put(out, &rc, 8);
    put(out, pairs.use(), pairs.size);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u %u\n", ck_sketch::SKETCH_SEG, ck_sketch::SKETCH_WAVES, ck_prealign::PREALIGN_WAVES);
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
        const int rc = kind == KIND_ANCHORS ? anchors_case(in, out, c) : kind == KIND_VOTES ? votes_case(in, out, c) : labels_case(in, out, c);
        if (rc) return rc;
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
