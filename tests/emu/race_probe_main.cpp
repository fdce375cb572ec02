// The schedules' own probe (TEST INFRASTRUCTURE ONLY, a host program: never compiled for the device, never linked into the
// product).  Four small LDS protocols written against ck:: alone, each in a form that holds its sync and a form that leaves it
// out; the unsynced forms are the bugs the fiber schedules of tests/emu/emu.cpp exist to find, and exist here only.  Linked against
// libcanon_emu.so for the scheduler; the schedule comes from the environment (CK_EMU_SCHEDULE), set by tests/emu/race_probe.py.
//   race_probe_main            one line per routine and form: "<routine> <synced|unsynced> <n> <n values>"
//   race_probe_main --skip K   a workgroup of two waves in which somebody skips a collective (K = 0: one lane a wave collective, 1: a
//                              whole wave a barrier, 2: one lane a barrier, 3: one lane takes barrier and collective in the other
//                              order): the emulator must report the deadlock and abort, under every schedule
// What each routine must give is restated in plain Python in tests/test_race_probe_cpu.py.
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

namespace {

constexpr uint32_t STALE = 0xDEAD0000u;         // what a slot holds before anybody has written it
constexpr uint32_t ROUNDS = 4, WG = 128;

struct Probe { bool synced; std::vector<uint32_t> lds, out; };

uint32_t value(uint32_t round, uint32_t t) { return 1000u * (round + 1) + 3u * t + 7u; }

// (a) neighbour exchange inside one wave: lane l writes a[l], then reads a[l ^ 1] and a[(l + 1) & 63].  The sync separates every
// lane's write from its neighbours' reads.  out[2l], out[2l + 1].
void exchange(void* p)
{
    Probe* P = (Probe*)p;
    const uint32_t l = ck::lane_id();
    uint32_t* a = P->lds.data();
    a[l] = value(0, l);
    if (P->synced) ck::wave_sync();
    P->out[2 * l] = a[l ^ 1];
    P->out[2 * l + 1] = a[(l + 1) & 63];
}

// (b) a producer wave and a consumer wave: thread l of the producer writes buf[l], thread l of the consumer reads buf[63 - l].
// The barrier is the only thing between the two waves.  UP: wave 0 produces for wave 1; otherwise wave 1 for wave 0.  out[l].
template <bool UP>
void produce_consume(void* p)
{
    Probe* P = (Probe*)p;
    const uint32_t l = ck::lane_id(), producer = UP ? 0u : 1u;
    uint32_t* buf = P->lds.data();
    if (ck::wave_in_block() == producer) buf[l] = value(0, l);
    if (P->synced) ck::block_barrier();
    if (ck::wave_in_block() != producer) P->out[l] = buf[63 - l];
}

// (c) a buffer reused in a loop: every round lane l writes buf[l], syncs, and reads its upper neighbour's slot (lane 63 has none).
// The trailing sync keeps the next round's write behind this round's reads -- the write-after-read case.  out[l] = the sum over
// the rounds of (round + 1) * what was read.
void reuse(void* p)
{
    Probe* P = (Probe*)p;
    const uint32_t l = ck::lane_id();
    uint32_t* buf = P->lds.data();
    uint32_t acc = 0;
    for (uint32_t r = 0; r < ROUNDS; ++r) {
        buf[l] = value(r, l);
        ck::wave_sync();
        acc += (r + 1) * (l < 63 ? buf[l + 1] : 0u);
        if (P->synced) ck::wave_sync();
    }
    P->out[l] = acc;
}

// (d) a Hillis-Steele doubling scan over WG threads (two waves) with three barriers a step; the unsynced form leaves out the
// middle one, between every thread's read of lds[tid - d] and every thread's write of lds[tid].  out[tid] = the sum in front of
// thread tid, out[WG + tid] = the total as thread tid sees it.
void doubling(void* p)
{
    Probe* P = (Probe*)p;
    const uint32_t tid = 64 * ck::wave_in_block() + ck::lane_id();
    uint32_t* lds = P->lds.data();
    lds[tid] = value(0, tid);
    ck::block_barrier();
    for (uint32_t d = 1; d < WG; d <<= 1) {
        const uint32_t prev = tid >= d ? lds[tid - d] : 0u;
        if (P->synced) ck::block_barrier();
        lds[tid] = prev + lds[tid];
        ck::block_barrier();
    }
    P->out[tid] = tid ? lds[tid - 1] : 0u;
    P->out[WG + tid] = lds[WG - 1];
    ck::block_barrier();
}

void skipper(void* p)
{
    const int k = *(const int*)p;
    const uint32_t l = ck::lane_id(), w = ck::wave_in_block();
    if (k == 0) { if (!(w == 1 && l == 5)) ck::wave_sync(); }
    if (k == 1) { ck::wave_sync(); if (w != 0) ck::block_barrier(); }
    if (k == 2) { if (!(w == 0 && l == 63)) ck::block_barrier(); ck::wave_sync(); }
    if (k == 3) { if (w == 0 && l == 7) ck::block_barrier(); else { ck::wave_sync(); ck::block_barrier(); } ck::wave_sync(); }
}

struct Routine { const char* name; void (*body)(void*); int nwaves; size_t n_out; };
const Routine kRoutines[] = {
    { "exchange", exchange, 1, 128 },
    { "produce_up", produce_consume<true>, 2, 64 },
    { "produce_down", produce_consume<false>, 2, 64 },
    { "reuse", reuse, 1, 64 },
    { "doubling", doubling, 2, 2 * WG },
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 3 && !strcmp(argv[1], "--skip")) {
        int k = atoi(argv[2]);
        ck::emu::run_block(skipper, &k, 2);
        printf("finished\n");                   // (never: run_block aborts)
        return 0;
    }
    for (const Routine& r : kRoutines)
        for (int synced = 1; synced >= 0; --synced) {
            Probe P{ synced != 0, std::vector<uint32_t>(WG, STALE), std::vector<uint32_t>(r.n_out, STALE) };
            ck::emu::run_block(r.body, &P, r.nwaves);
            printf("%s %s %zu", r.name, synced ? "synced" : "unsynced", r.n_out);
            for (uint32_t v : P.out) printf(" %u", v);
            printf("\n");
        }
    return 0;
}
