// CPU fiber run of the cluster unit (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that compiles
// circkit_amd/csrc/cluster.h and ck_scan.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler.  It reads a file of cases and writes a file of results (formats: tests/emu/cluster_emu.py).  A candidates case runs
// keys_lane() as every lane of its grid, finds the smallest position of every key with a std::map (the product asks the uniq
// unit, which is not this unit's code), runs count_wave() as every wave of its grid, the three bodies of the scan as workgroups
// of the product's SCAN_WG threads, and write_wave(); a link case runs init_lane(), link_lane() and flatten_lane() as every lane
// of their grids.  A lane that skips a collective deadlocks its wave, and UBSan + bounds checks watch every shift and access.
// The rows, the keys, the positions, the masks, the offsets, the pairs, the scores, the parents and the labels each lie in an
// exactly sized heap block between canaries, and every input is compared with its copy afterwards.
//   cluster_emu_main --constants          prints "SCAN_WG SCAN_ITEMS"
//   cluster_emu_main CASES RESULTS
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/ck_scan.h"
#include "../../circkit_amd/csrc/cluster.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
constexpr int SCAN_WG = (int)ck_cluster::SCAN_WG, SCAN_ITEMS = (int)ck_cluster::SCAN_ITEMS;
enum { RC_OK = 0, RC_CANARY = 2 };
enum { KIND_CANDIDATES = 0, KIND_LINK = 1 };

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

uint32_t tid() { return 64 * ck::wave_in_block() + ck::lane_id(); }

struct KeysLaunch { ck_cluster::Keys K; uint64_t wave, n_waves; };
void keys_body(void* p) { KeysLaunch* L = (KeysLaunch*)p; ck_cluster::keys_lane(L->K, L->wave * 64 + ck::lane_id(), L->n_waves * 64); }

struct EmitLaunch { ck_cluster::Emit E; uint64_t wave, n_waves; };
void count_body(void* p) { EmitLaunch* L = (EmitLaunch*)p; ck_cluster::count_wave(L->E, L->wave, L->n_waves); }
void write_body(void* p) { EmitLaunch* L = (EmitLaunch*)p; ck_cluster::write_wave(L->E, L->wave, L->n_waves); }

struct ScanLaunch { uint64_t* a; uint64_t n, tile, n_tiles; uint64_t* sums; uint64_t* lds; uint64_t total; };
void tile_sums_body(void* p)
{
    ScanLaunch* L = (ScanLaunch*)p;
    const uint64_t t = ck_scan::tile_sum<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(tid(), L->tile, L->a, L->n, [](uint64_t w) { return w; }, L->lds);
    if (tid() == 0) L->sums[L->tile] = t;
}
void scan_sums_body(void* p)
{
    ScanLaunch* L = (ScanLaunch*)p;
    const uint64_t t = ck_scan::sums_exclusive<SCAN_WG, ck_scan::SatAdd>(tid(), L->sums, L->n_tiles, L->lds);
    if (tid() == 0) L->total = t;
}
void apply_body(void* p)
{
    ScanLaunch* L = (ScanLaunch*)p;
    ck_scan::apply_ends<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(tid(), L->tile, L->a, L->n, L->sums, L->lds);
}

struct LinkLaunch { ck_cluster::Link L; uint64_t wave, n_waves; };
void init_body(void* p) { LinkLaunch* L = (LinkLaunch*)p; ck_cluster::init_lane(L->L, L->wave * 64 + ck::lane_id(), L->n_waves * 64); }
void link_body(void* p) { LinkLaunch* L = (LinkLaunch*)p; ck_cluster::link_lane(L->L, L->wave * 64 + ck::lane_id(), L->n_waves * 64); }
void flatten_body(void* p) { LinkLaunch* L = (LinkLaunch*)p; ck_cluster::flatten_lane(L->L, L->wave * 64 + ck::lane_id(), L->n_waves * 64); }

int candidates_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[7];     // n_records, log2_bins, n_bands, band_bins, capacity, waves of the keys kernel, waves of the count / write kernels
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0], bins = 1ull << h[1], nb = h[2], capacity = h[4], n_keys = n * nb;
    Block rows(n * bins * 8, IN_CANARY);
    if (!get(in, rows.use(), rows.size)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
    const std::vector<uint8_t> rows0(rows.use(), rows.use() + rows.size);
    const uint64_t tiles = (n + ck_cluster::SCAN_TILE - 1) / ck_cluster::SCAN_TILE;
    Block keys(n_keys * 8, OUT_CANARY), first(n_keys * 8, OUT_CANARY), masks(n * 8, OUT_CANARY), offsets((n + 1) * 8, OUT_CANARY),
        pairs(capacity * 8, OUT_CANARY), sums(tiles * 8, OUT_CANARY), lds(SCAN_WG * 8, OUT_CANARY);

    KeysLaunch KL;
    KL.K.rows = (const uint64_t*)rows.use(); KL.K.n_records = n; KL.K.log2_bins = (uint32_t)h[1]; KL.K.n_bands = (uint32_t)nb;
    KL.K.band_bins = (uint32_t)h[3]; KL.K.keys = (uint64_t*)keys.use();
    KL.n_waves = h[5];
    for (KL.wave = 0; n && KL.wave < KL.n_waves; ++KL.wave) ck::emu::run_block(keys_body, &KL, 1);
    // the uniq unit's answer: the smallest position with an equal key
    {
        std::map<uint64_t, uint64_t> seen;
        const uint64_t* k = (const uint64_t*)keys.use();
        uint64_t* f = (uint64_t*)first.use();
        for (uint64_t p = 0; p < n_keys; ++p) f[p] = seen.emplace(k[p], p).first->second;
    }
    const std::vector<uint8_t> keys0(keys.use(), keys.use() + keys.size), first0(first.use(), first.use() + first.size);

    EmitLaunch EL;
    EL.E.keys = (const uint64_t*)keys.use(); EL.E.first_pos = (const uint64_t*)first.use(); EL.E.n_records = n; EL.E.n_bands = (uint32_t)nb;
    EL.E.masks = (uint64_t*)masks.use(); EL.E.offsets = (uint64_t*)offsets.use(); EL.E.pairs = (uint32_t*)pairs.use(); EL.E.capacity = capacity;
    EL.n_waves = h[6];
    for (EL.wave = 0; n && EL.wave < EL.n_waves; ++EL.wave) ck::emu::run_block(count_body, &EL, 1);
    ScanLaunch SL;
    SL.a = (uint64_t*)offsets.use() + 1; SL.n = n; SL.n_tiles = tiles; SL.sums = (uint64_t*)sums.use(); SL.lds = (uint64_t*)lds.use(); SL.total = 0;
    for (SL.tile = 0; SL.tile < tiles; ++SL.tile) ck::emu::run_block(tile_sums_body, &SL, SCAN_WG / 64);
    ck::emu::run_block(scan_sums_body, &SL, SCAN_WG / 64);
    ((uint64_t*)offsets.use())[0] = 0;
    for (SL.tile = 0; SL.tile < tiles; ++SL.tile) ck::emu::run_block(apply_body, &SL, SCAN_WG / 64);
    for (EL.wave = 0; n && EL.wave < EL.n_waves; ++EL.wave) ck::emu::run_block(write_body, &EL, 1);

    uint64_t rc = RC_OK;
    if (!rows.intact() || !keys.intact() || !first.intact() || !masks.intact() || !offsets.intact() || !pairs.intact() || !sums.intact() ||
        !lds.intact() || changed(rows0, rows.use()) || changed(keys0, keys.use()) || changed(first0, first.use()))
        rc = RC_CANARY;
    const uint64_t r[2] = { rc, SL.total };
    put(out, r, sizeof r);
    put(out, keys.use(), keys.size);
    put(out, offsets.use(), offsets.size);
    put(out, pairs.use(), pairs.size);
    return 0;
}

int link_case(FILE* in, FILE* out, uint64_t c)
{
    uint64_t h[6];     // n_records, n_pairs, min_similarity_q16, min_filled, waves of the link kernel, waves of the init / flatten kernels
    if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
    const uint64_t n = h[0], m = h[1];
    Block pairs(m * 8, IN_CANARY), scores(m * 8, IN_CANARY), parent(n * 4, OUT_CANARY), labels(n * 8, OUT_CANARY);
    if (!get(in, pairs.use(), pairs.size) || !get(in, scores.use(), scores.size)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
    const std::vector<uint8_t> p0(pairs.use(), pairs.use() + pairs.size), s0(scores.use(), scores.use() + scores.size);
    uint64_t totals[ck_cluster::L_WORDS] = { 0, 0, 0 };
    LinkLaunch LL;
    LL.L.n_records = n; LL.L.pairs = (const uint32_t*)pairs.use(); LL.L.scores = (const uint32_t*)scores.use(); LL.L.n_pairs = m;
    LL.L.min_similarity_q16 = (uint32_t)h[2]; LL.L.min_filled = (uint32_t)h[3];
    LL.L.parent = (uint32_t*)parent.use(); LL.L.labels = (uint64_t*)labels.use(); LL.L.totals = totals;
    LL.n_waves = h[5];
    for (LL.wave = 0; n && LL.wave < LL.n_waves; ++LL.wave) ck::emu::run_block(init_body, &LL, 1);
    LL.n_waves = h[4];
    for (LL.wave = 0; m && LL.wave < LL.n_waves; ++LL.wave) ck::emu::run_block(link_body, &LL, 1);
    LL.n_waves = h[5];
    for (LL.wave = 0; n && LL.wave < LL.n_waves; ++LL.wave) ck::emu::run_block(flatten_body, &LL, 1);
    uint64_t rc = RC_OK;
    if (!pairs.intact() || !scores.intact() || !parent.intact() || !labels.intact() || changed(p0, pairs.use()) || changed(s0, scores.use()))
        rc = RC_CANARY;
    // the invariant of the parent array, on what the link left behind
    for (uint64_t i = 0; i < n; ++i) if (((const uint32_t*)parent.use())[i] > i) rc = RC_CANARY;
    const uint64_t r[4] = { rc, totals[ck_cluster::L_CLUSTERS], totals[ck_cluster::L_LINKED], totals[ck_cluster::L_INVALID] };
    put(out, r, sizeof r);
    put(out, labels.use(), labels.size);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u\n", ck_cluster::SCAN_WG, ck_cluster::SCAN_ITEMS);
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
        const int rc = kind == KIND_CANDIDATES ? candidates_case(in, out, c) : link_case(in, out, c);
        if (rc) return rc;
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
