// CPU fiber run of the monomerize wave routine (TEST INFRASTRUCTURE ONLY, never linked into the product): compiles
// circkit_amd/csrc/monomerize.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler (ck::emu::run_block, gather, cur_lane, ...), so a lane that skips a collective deadlocks the wave and is
// reported, and UBSan + bounds checks watch every shift and access of the kernel source.
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/monomerize.h"

namespace {
struct Launch { const uint8_t* s; uint32_t n; ck_mono::Params P; uint32_t res[64]; };
void body(void* p)
{
    Launch* L = (Launch*)p;
    L->res[ck::lane_id()] = ck_mono::record_end(L->s, L->n, L->P);
}
}  // namespace

// out[i] = the end index of record i as the kernel would store it; returns -1 when the lanes of a wave disagree, -2 for a
// record of 2^32 bytes or more
extern "C" int emu_monomerize_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, uint32_t seed_len,
                                    uint32_t use_identity, uint64_t overlap_dist, double min_identity, uint32_t sensitive,
                                    uint32_t* out)
{
    for (uint64_t i = 0; i < n_records; ++i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len > 0xFFFFFFFFull) return -2;
        Launch L;
        L.s = bytes + offsets[i];
        L.n = (uint32_t)len;
        L.P.overlap_dist = overlap_dist; L.P.min_identity = min_identity;
        L.P.seed_len = seed_len; L.P.use_identity = use_identity; L.P.sensitive = sensitive;
        ck::emu::run_block(body, &L, 1);
        for (int l = 1; l < 64; ++l) if (L.res[l] != L.res[0]) return -1;
        out[i] = L.res[0];
    }
    return 0;
}
