// A payload `lead` bytes into its buffer, for the CPU fiber programs (TEST INFRASTRUCTURE ONLY, never linked into the product).
// The kernel under test gets use() as its `bytes` and offsets that begin at `lead`.  Below HIGH_LEAD the buffer is a heap block
// filled with the canary, the lead region included, and all of it is watched.  From HIGH_LEAD on -- a GiB and more: the leads that put
// a payload across byte 2^32 of its buffer -- the buffer is an anonymous mapping that the system reserves lazily: the lead region is
// neither touched nor copied (it reads as zeros, which is what a position truncated to 32 bits then finds), canaries surround the
// payload only, and only that window is watched.
#ifndef CK_EMU_LEAD_BLOCK_H
#define CK_EMU_LEAD_BLOCK_H
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <vector>

namespace ck_emu {

constexpr uint64_t HIGH_LEAD = 1ull << 30;

struct LeadBlock {
    static constexpr size_t GUARD = 64;
    uint8_t* raw = nullptr;
    size_t shift, lead, nb, bytes;
    bool high;
    std::vector<uint8_t> before;
    LeadBlock(size_t shift_, uint64_t lead_, size_t nb_, uint8_t canary) : shift(shift_), lead((size_t)lead_), nb(nb_), high(lead_ >= HIGH_LEAD)
    {
        bytes = GUARD + shift + lead + nb + GUARD;
        if (high) {
            raw = (uint8_t*)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
            if (raw == (uint8_t*)MAP_FAILED) abort();
            memset(window(), canary, window_bytes());
        } else {
            if (posix_memalign((void**)&raw, 64, bytes)) abort();
            memset(raw, canary, bytes);
        }
    }
    LeadBlock(const LeadBlock&) = delete;
    ~LeadBlock() { if (high) munmap(raw, bytes); else free(raw); }
    uint8_t* use() { return raw + GUARD + shift; }                  // `shift` past a 64-byte boundary
    uint8_t* payload() { return use() + lead; }
    uint8_t* window() { return high ? payload() - GUARD : raw; }    // what is watched
    size_t window_bytes() const { return high ? GUARD + nb + GUARD : bytes; }
    void keep() { before.assign(window(), window() + window_bytes()); }                    // call once the payload is in place
    bool unchanged() { return before.size() == window_bytes() && !memcmp(before.data(), window(), window_bytes()); }
};

}  // namespace ck_emu
#endif
