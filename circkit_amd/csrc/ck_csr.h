// ck_csr.h -- the walk over the offsets of a host CSR batch (internal; no HIP: tests/san/csr_san_main.cpp builds it alone).
//
// Every host-buffer entry point reads offsets[0 .. n] before it reads a payload byte or enqueues anything.  What is wrong with
// them is found here once; the unit keeps its own messages, its own limit and its own check of offsets[0].
#pragma once
#include <stdint.h>

enum ck_csr_fault { CK_CSR_OK, CK_CSR_DECREASE, CK_CSR_TOO_LONG };
constexpr uint64_t CK_CSR_NO_LIMIT = 0;      // (no record has a length below 0, so 0 is free to mean none)

// The first record i of offsets[0 .. n] that is at fault, in *at (left alone without one): offsets[i + 1] < offsets[i], or a
// length that reaches `limit` (exclusive).  A record with both is a decrease.
inline ck_csr_fault ck_csr_walk(const uint64_t* offsets, uint64_t n, uint64_t limit, uint64_t* at)
{
    for (uint64_t i = 0; i < n; ++i) {
        const bool decrease = offsets[i + 1] < offsets[i];
        if (decrease || (limit && offsets[i + 1] - offsets[i] >= limit)) {
            *at = i;
            return decrease ? CK_CSR_DECREASE : CK_CSR_TOO_LONG;
        }
    }
    return CK_CSR_OK;
}
