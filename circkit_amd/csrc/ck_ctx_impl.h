// ck_ctx_impl.h -- struct circkit_ctx with all its fields (internal).  Included by the two units that own them and by nobody else:
// circkit_hip.hip (create, destroy, the stream, the accessors of ck_ctx.h) and circkit_canon.hip (the canonicalize state, which is
// allocated with the ctx and not behind a unit slot).  Every other unit sees the ctx through ck_ctx.h.
#pragma once
#include <string>

#include "canon_config.h"      // N_TIERS: one deferral list per stage
#include "ck_ctx.h"

// circkit_canon.hip: what its kernels need set once per ctx (the last step of circkit_ctx_create)
int ck_canon_init(circkit_ctx* c);

struct circkit_ctx {
    int device = -1;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t ev_order = nullptr;       // circkit_ctx_set_stream: the new stream waits for what the ctx queued on the old one
    // host-buffer batches in parts (host_batch): copy-in and copy-out streams of the ctx's own and one event pair per part, so
    // that part k + 1 arrives and part k - 1 leaves while part k computes (PCIe is full duplex)
    static constexpr int MAX_PARTS = 32;
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[MAX_PARTS] = {}, ev_done[MAX_PARTS] = {}, ev_head = nullptr;
    bool timed = false;
    std::string err;
    uint8_t* d_comp = nullptr;
    uint32_t* d_counters = nullptr;      // [3] unprocessed records
    // segmented deferral lists: streaming kernel -> rescue pass / mixed kernel -> stage A -> stage C -> team stage -> global
    // stage (one segment per producing workgroup)
    uint32_t* d_lists[N_TIERS + 1] = {}; // [0] streaming kernel -> rescue pass, [i + 1] input list of tier i (output of the stage before)
    uint32_t* d_seg_counts = nullptr;    // [(N_TIERS + 1) * seg_alloc]
    uint64_t list_cap = 0, seg_alloc = 0;
    // host-batch staging (grow only)
    uint8_t *d_in = nullptr, *d_out = nullptr, *d_strand = nullptr;
    uint64_t* d_off = nullptr; uint32_t* d_idx = nullptr; uint64_t* d_hash = nullptr;
    uint64_t cap_bytes = 0, cap_rec = 0;
    ck_buf<uint32_t> d_view;             // hash-only batches: strand + rotation of the records whose hash is not fused
    ck_buf<uint8_t> d_hashed;            // per record: hash already written by the streaming kernel
    // records beyond the last LDS tier run the same per-record code over slices of this global-memory scratch
    // (grow-only; the device API allocates the default on first use, the host API sizes it for the batch's longest record)
    ck_buf<uint8_t> d_gscratch;          // (its capacity in bytes; the kernels take it as words)
    uint64_t gscratch_default = 256ull << 20;
    // the previous batch's mode (1 / 2 / 3, see stream_mode): only picks which build gets the full-size grid
    uint64_t* h_off = nullptr;           // page-locked staging of a host batch's offsets and per-record outputs (host_batch): h_off_cap x (8 + 8 + 4 + 1) bytes
    uint64_t h_off_cap = 0;
    volatile uint32_t* h_mode = nullptr; // pinned host word the rescue kernel writes the batch's mode to (d_mode = its device address)
    uint32_t* d_mode = nullptr;
    uint32_t mode_seen = 0;                   // launch_canon: the mode word as the previous device batch's launch read it (MODE_GUESS)
    // the other units' state (ck_ctx.h): each puts its state in its slot and names the function that deletes it
    struct { void* p; void (*release)(void*); } units[CK_N_UNITS] = {};
};
