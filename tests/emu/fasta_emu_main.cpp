// CPU fiber run of the device FASTA parser (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that
// compiles circkit_amd/csrc/fasta_device.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler.  It reads a file of cases and writes a file of results (formats: tests/emu/fasta_emu.py).  Per case the steps of
// circkit_fasta.hip run in their order: scan_bounds16 per 16 bytes and the two maxima, resolve_bounds, summarize_tile as a
// workgroup of the product's WAVES waves per tile, the scan over the summaries as plain host code with the kernel's two rules
// (next_state, tile_kept; the scan kernel uses no wave routine), verdict, apply_tile as a workgroup per tile, finish_spans per
// record.  A lane that skips a collective deadlocks its wave; UBSan + bounds checks watch every shift and access.  The text,
// the payload, the offsets and both span arrays each lie in an exactly sized heap block between canaries.
//   fasta_emu_main --constants          prints "TILE_BYTES SCAN_WG WAVES"
//   fasta_emu_main CASES RESULTS
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

#include "../../circkit_amd/csrc/fasta_device.h"
#include "../../circkit_amd/csrc/fasta_host.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_CANARY = 2 };

struct Launch {
    ck_fasta::Text T;
    ck_fasta::Apply A;
    uint64_t tile;
    ck_fasta::Shared* S;
    ck_fasta::Summary* summary;
};
void summarize_body(void* p)
{
    Launch* L = (Launch*)p;
    ck_fasta::summarize_tile(L->T, L->tile, *L->S, L->summary);
}
void apply_body(void* p)
{
    Launch* L = (Launch*)p;
    ck_fasta::apply_tile(L->A, L->tile, *L->S);
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
        printf("%u %u %u\n", ck_fasta::TILE_BYTES, ck_fasta::SCAN_WG, ck_fasta::WAVES);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULTS | --constants\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }
    ck_fasta::Shared* S = new ck_fasta::Shared();
    memcpy(S->lut, ckhost::normalize_lut(), 256);          // as the ctx slot copies it to the device

    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t h[6];                                     // n, flags (1 first, 2 final), in_shift, out_shift, record capacity, byte capacity (~0: exact)
        if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
        const uint64_t n = h[0];
        Block text(h[2], n, IN_CANARY);
        if (!get(in, text.use(), n)) { fprintf(stderr, "case %llu: short body\n", (unsigned long long)c); return 2; }
        const std::vector<uint8_t> before(text.use(), text.use() + n);

        uint64_t first_body = ~0ull, last_candidate = 0;
        for (uint64_t pos = 0; pos < n; pos += 16) ck_fasta::scan_bounds16(text.use(), n, pos, &first_body, &last_candidate);
        bool error;
        const ck_fasta::Text T = ck_fasta::resolve_bounds(text.use(), n, first_body, last_candidate, (h[1] & 1) != 0, (h[1] & 2) != 0, &error);

        const uint64_t tiles = (n + ck_fasta::TILE_BYTES - 1) / ck_fasta::TILE_BYTES;
        std::vector<ck_fasta::Summary> summaries(tiles ? tiles : 1);
        std::vector<ck_fasta::Prefix> prefix(tiles ? tiles : 1);
        Launch L;
        L.T = T; L.S = S;
        for (uint64_t t = 0; t < tiles; ++t) {
            L.tile = t; L.summary = &summaries[t];
            ck::emu::run_block(summarize_body, &L, (int)ck_fasta::WAVES);
        }
        uint64_t records = 0, bytes = 0;
        uint32_t state = ck_fasta::ST_SEQ;
        for (uint64_t t = 0; t < tiles; ++t) {
            prefix[t] = ck_fasta::Prefix{ records, bytes, state };
            records += summaries[t].starts;
            bytes += ck_fasta::tile_kept(summaries[t], state);
            state = ck_fasta::next_state(state, summaries[t].kind);
        }
        const uint64_t record_capacity = h[4] == ~0ull ? records : h[4], byte_capacity = h[5] == ~0ull ? bytes : h[5];
        Block payload(h[3], byte_capacity, OUT_CANARY);
        Block offsets(0, 8 * (record_capacity + 1), OUT_CANARY), head(0, 16 * record_capacity, OUT_CANARY), raw(0, 16 * record_capacity, OUT_CANARY);
        const uint32_t refused = error ? (uint32_t)ck_fasta::REFUSED_FORMAT
                                       : ck_fasta::verdict(records, bytes, record_capacity, byte_capacity, text.use(), n, payload.use());
        uint64_t* off = (uint64_t*)offsets.use();
        off[0] = 0;
        if (!refused) {
            off[records] = bytes;
            L.A.T = T; L.A.prefix = prefix.data();
            L.A.out = payload.use(); L.A.offsets = off;
            L.A.head = (ck_fasta::Span*)head.use(); L.A.raw = (ck_fasta::Span*)raw.use();
            if (records)
                for (uint64_t t = T.p0 / ck_fasta::TILE_BYTES; t < tiles && t * ck_fasta::TILE_BYTES < T.limit; ++t) {
                    L.tile = t;
                    ck::emu::run_block(apply_body, &L, (int)ck_fasta::WAVES);
                }
            for (uint64_t r = 0; r < records; ++r) ck_fasta::finish_spans(T, r, records, state == ck_fasta::ST_SEQ, L.A.head, L.A.raw);
        }
        const uint64_t R = refused ? 0 : records, B = refused ? 0 : bytes;
        uint64_t rc = RC_OK;
        if (!text.intact(n) || (n && memcmp(before.data(), text.use(), n)) || !payload.intact(B) || !offsets.intact(refused ? 8 : 8 * (R + 1)) ||
            !head.intact(16 * R) || !raw.intact(16 * R))
            rc = RC_CANARY;
        const uint64_t r[5] = { rc, refused, error ? 0 : records, error ? 0 : bytes, error ? 0 : T.limit };
        put(out, r, sizeof r);
        put(out, off, 8 * (R + 1));
        put(out, payload.use(), B);
        put(out, head.use(), 16 * R);
        put(out, raw.use(), 16 * R);
    }
    delete S;
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
