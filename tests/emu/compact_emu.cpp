// CPU fiber run of the monomer compact (TEST INFRASTRUCTURE ONLY, never linked into the product): compiles
// circkit_amd/csrc/monomer_compact.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler, as mono_emu.cpp does.  decide() runs per record as the decide kernel's lane would run it; the scan between the
// two is plain host code here (the scan kernels use no wave routine); gather_tile() runs as a workgroup of the product's
// GATHER_WAVES waves per output tile, so a lane that skips a collective deadlocks its wave and UBSan + bounds checks watch
// every shift and access.
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include <vector>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/monomer_compact.h"

namespace {
struct Launch {
    ck_compact::Gather G;
    uint64_t tile;
    uint64_t first[ck_compact::GATHER_WAVES][64];
};
void body(void* p)
{
    Launch* L = (Launch*)p;
    ck_compact::gather_tile(L->G, L->tile, &L->first[ck::wave_in_block()][ck::lane_id()]);
}
}  // namespace

extern "C" uint32_t emu_compact_tile_bytes() { return ck_compact::TILE_BYTES; }
extern "C" uint32_t emu_compact_waves() { return ck_compact::GATHER_WAVES; }

// The compact of one batch.  out_offsets (n + 1), out_src (n) and kept_end (n) as the device form writes them; *n_kept = m.
// Returns 0, or -1 when the lanes of a wave disagree on the record their search found.
extern "C" int emu_monomers_compact(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const uint32_t* end, const uint64_t* full_len,
                                    uint64_t min_length, uint64_t max_length, uint64_t min_overlap, double min_overlap_percent,
                                    uint32_t use_percent, uint32_t keep_all, uint8_t* out_bytes, uint64_t* out_offsets, uint64_t* out_src,
                                    uint32_t* kept_end, uint64_t* n_kept)
{
    ck_compact::Filter F;
    F.min_length = min_length; F.max_length = max_length; F.min_overlap = min_overlap;
    F.min_overlap_percent = min_overlap_percent; F.use_percent = use_percent; F.keep_all = keep_all;
    std::vector<uint64_t> src_start(n ? n : 1);
    uint64_t m = 0, B = 0;
    out_offsets[0] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        const uint64_t w = ck_compact::decide(len, full_len ? full_len[i] : len, end[i], F, &kept_end[i]);
        if (!(w & ck_compact::WRITTEN)) continue;
        B += w & ~ck_compact::WRITTEN;
        out_offsets[m + 1] = B;
        out_src[m] = i;
        src_start[m] = offsets[i];
        ++m;
    }
    *n_kept = m;
    if (n == 0 || B == 0) return 0;
    Launch L;
    L.G.bytes = bytes; L.G.p0 = offsets[0]; L.G.p1 = offsets[n];
    L.G.out_offsets = out_offsets; L.G.src_start = src_start.data();
    L.G.m = m; L.G.B = B; L.G.out = out_bytes;
    const uint64_t n_gran = (((uint64_t)(uintptr_t)out_bytes & 15u) + B + 15) / 16;
    const uint64_t n_tiles = (n_gran + ck_compact::TILE_GRANULES - 1) / ck_compact::TILE_GRANULES;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        L.tile = t;
        for (auto& wv : L.first) for (uint64_t& x : wv) x = ~0ull;
        ck::emu::run_block(body, &L, (int)ck_compact::GATHER_WAVES);
        for (auto& wv : L.first)
            for (int l = 1; l < 64; ++l) if (wv[l] != wv[0]) return -1;
    }
    return 0;
}
