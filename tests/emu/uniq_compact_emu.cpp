// Host run of the uniq compact's decision (TEST INFRASTRUCTURE ONLY, never linked into the product): compiles
// circkit_amd/csrc/monomer_compact.h against tests/emu/wave_prims_emu.h, as compact_emu.cpp does, and runs
// ck_compact::decide_uniq per record as the decide kernel's lane runs it.  The scan and the gather behind it are the monomer
// compact's, which compact_emu.cpp runs as fibers.
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include "../../circkit_amd/csrc/wave_prims.h"
#include "../../circkit_amd/csrc/monomer_compact.h"

extern "C" uint64_t emu_uniq_written_bit() { return ck_compact::WRITTEN; }

// w[i] for n records of the given lengths
extern "C" void emu_uniq_decide(const uint64_t* lengths, const uint64_t* first_seen, uint64_t base, uint64_t n, uint64_t* w)
{
    for (uint64_t i = 0; i < n; ++i) w[i] = ck_compact::decide_uniq(lengths[i], first_seen[i], base, i);
}
