// CPU fiber run of the op table of the wave primitives (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone
// program that compiles tests/prims/prims_ops.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler.  It reads a file of cases and writes a file of results (formats: tests/emu/prims_emu.py).  Every case runs as one
// workgroup of NWAVES waves that all run the case, like the device probe (tests/prims/prims_probe.hip): each wave has results,
// global memory and an LDS slice of its own; the LDS slices and the workgroup's exchange words lie between canaries.
//   prims_emu_main NWAVES CASES RESULTS
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

#include "../prims/prims_ops.h"

namespace {

using namespace ck_prims;
constexpr size_t GUARD = 64;                                           // dwords of canary on either side of an LDS array
constexpr uint32_t CANARY = 0xA5A5A5A5u;

struct Block {
    uint32_t op = 0, mode = 0, nwaves = 1;
    std::vector<uint32_t> in, out, lds, xchg;                          // in: 64 x IN_W; out: nwaves x 64 x OUT_W
    std::vector<uint8_t*> mem;                                         // per wave: MEM_BYTES on a 4 KiB boundary
    uint32_t* lds_of(uint32_t w) { return lds.data() + GUARD + (size_t)w * (LDS_DW + GUARD); }
    bool intact() const
    {
        for (size_t k = 0; k < GUARD; ++k) {
            for (uint32_t w = 0; w <= nwaves; ++w)
                if (lds[(size_t)w * (LDS_DW + GUARD) + k] != CANARY) return false;
            if (xchg[k] != CANARY || xchg[GUARD + XCHG_DW + k] != CANARY) return false;
        }
        return true;
    }
};

void body(void* p)
{
    Block* b = (Block*)p;
    const uint32_t w = ck::emu::cur_wave(), t = ck::emu::cur_lane();
    const uint32_t* in = b->in.data() + (size_t)t * IN_W;
    uint32_t* out = b->out.data() + ((size_t)w * 64 + t) * OUT_W;
    if (b->mode) run_case<1>(b->op, in, out, b->mem[w], b->lds_of(w), b->xchg.data() + GUARD, b->nwaves);
    else run_case<0>(b->op, in, out, b->mem[w], b->lds_of(w), b->xchg.data() + GUARD, b->nwaves);
}

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s NWAVES CASES RESULTS\n", argv[0]); return 2; }
    const int nwaves = atoi(argv[1]);
    if (nwaves < 1 || nwaves > 16) { fprintf(stderr, "NWAVES is 1..16\n"); return 2; }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) { perror("open"); return 2; }
    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    Block b;
    b.nwaves = (uint32_t)nwaves;
    b.in.resize(64 * IN_W);
    b.out.resize((size_t)nwaves * 64 * OUT_W);
    uint8_t* pool = nullptr;                                           // guard page, nwaves x MEM_BYTES, guard page
    const size_t pool_bytes = 4096 + (size_t)nwaves * MEM_BYTES + 4096;
    if (posix_memalign((void**)&pool, 4096, pool_bytes)) return 3;
    for (int w = 0; w < nwaves; ++w) b.mem.push_back(pool + 4096 + (size_t)w * MEM_BYTES);
    std::vector<uint8_t> image(MEM_BYTES);
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint32_t h[4];                                                 // op, mode, has memory, 0
        if (!get(in, h, sizeof h) || !get(in, b.in.data(), 4 * b.in.size())) { fprintf(stderr, "case %llu: short case\n", (unsigned long long)c); return 2; }
        memset(image.data(), 0, MEM_BYTES);
        if (h[2] && !get(in, image.data(), MEM_BYTES)) { fprintf(stderr, "case %llu: short memory\n", (unsigned long long)c); return 2; }
        b.op = h[0]; b.mode = h[1];
        memset(pool, 0xA5, pool_bytes);
        for (int w = 0; w < nwaves; ++w) memcpy(b.mem[w], image.data(), MEM_BYTES);
        b.lds.assign(GUARD + (size_t)nwaves * (LDS_DW + GUARD), CANARY);
        b.xchg.assign(GUARD + XCHG_DW + GUARD, CANARY);
        std::fill(b.out.begin(), b.out.end(), 0xEEEEEEEEu);
        const std::vector<uint32_t> in_before = b.in;
        ck::emu::run_block(body, &b, nwaves);
        uint32_t rc = b.intact() && in_before == b.in ? 0u : 1u;
        for (size_t k = 0; k < 4096; ++k)
            if (pool[k] != 0xA5 || pool[pool_bytes - 1 - k] != 0xA5) rc |= 2u;
        put(out, b.out.data(), 4 * b.out.size());
        if (h[2]) put(out, pool + 4096, (size_t)nwaves * MEM_BYTES);
        put(out, &rc, 4);
    }
    free(pool);
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
