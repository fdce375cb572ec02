// ck_ctx_impl.h -- struct circkit_ctx with all its fields (internal).  Included by the two units that own them and by nobody else:
// circkit_hip.hip (create, destroy, the stream, the accessors of ck_ctx.h) and circkit_canon.hip (the canonicalize state, which is
// allocated with the ctx and not behind a unit slot).  Every other unit sees the ctx through ck_ctx.h.
#pragma once
#include <string>

#include "canon_plan.h"        // N_TIERS: one deferral list per stage; the words of d_counters and h_mode
#include "ck_ctx.h"

// circkit_canon.hip: what its kernels need set once per ctx (the last step of circkit_ctx_create)
int ck_canon_init(circkit_ctx* c);

struct circkit_ctx {
    int device = -1;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_order = nullptr;       // circkit_ctx_set_stream: the new stream waits for what the ctx queued on the old one
    // host-buffer batches in parts (host_batch): a copy-out stream of the ctx's own and one event per part, so that part k + 1
    // arrives and part k - 1 leaves while part k computes (PCIe is full duplex)
    static constexpr int MAX_PARTS = 32;
    hipStream_t s_out = nullptr;
    hipEvent_t ev_done[MAX_PARTS] = {}, ev_head = nullptr;
    bool timed = false;
    std::string err;
    ck_buf<uint8_t> d_comp;              // the complement table, 256 bytes
    ck_buf<uint32_t> d_counters;         // CTR_WORDS words (canon_plan.h CounterWord)
    // segmented deferral lists: streaming kernel -> rescue pass / mixed kernel -> stage A -> stage C -> team stage -> global
    // stage (one segment per producing workgroup)
    ck_buf<uint32_t> d_lists[N_TIERS + 1];   // [0] streaming kernel -> rescue pass, [i + 1] input list of tier i (output of the stage before)
    ck_buf<uint32_t> d_seg_counts;       // [(N_TIERS + 1) * seg_alloc]
    uint64_t seg_alloc = 0;
    // host-batch staging (grow only; ensure_staging): payload in and out, and one entry per record
    ck_buf<uint8_t> d_in, d_out, d_strand;
    ck_buf<uint64_t> d_off, d_hash;
    ck_buf<uint32_t> d_idx;
    ck_buf<uint32_t> d_view;             // hash-only batches: strand + rotation of the records whose hash is not fused
    ck_buf<uint8_t> d_hashed;            // per record: hash already written by the streaming kernel
    // records beyond the last LDS tier run the same per-record code over slices of this global-memory scratch
    // (grow-only; the device API allocates the default on first use, the host API sizes it for the batch's longest record)
    ck_buf<uint8_t> d_gscratch;          // (its capacity in bytes; the kernels take it as words)
    uint64_t gscratch_default = 256ull << 20;
    ck_pinned<uint8_t> h_stage;          // page-locked staging of a host batch's offsets and per-record outputs (host_batch): (8 + 8 + 4 + 1) bytes a record
    // pinned, mapped words the kernels write and the host reads without waiting (canon_plan.h HostWord): the previous batch's
    // mode only picks which build gets the full-size grid
    ck_pinned<volatile uint32_t> h_mode;
    uint32_t* d_mode = nullptr;          // their device address
    uint32_t mode_seen = 0;                   // launch_canon: the mode word as the previous device batch's launch read it (MODE_GUESS)
    // the other units' state (ck_ctx.h): each puts its state in its slot and names the function that deletes it
    struct { void* p; void (*release)(void*); } units[CK_N_UNITS] = {};
};
