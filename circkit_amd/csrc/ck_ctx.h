// ck_ctx.h -- what a translation unit other than circkit_hip.hip may ask of the ctx (internal; not part of the C ABI).
//
// struct circkit_ctx lives in circkit_hip.hip and nothing outside that file names one of its fields.  The other units
// (circkit_orfs.hip, circkit_monomerize.hip, circkit_uniq.hip, circkit_uniq_compact.hip, circkit_windows.hip, circkit_fasta.hip, circkit_fasta_write.hip, circkit_sketch.hip) enqueue on the ctx's stream, report through its error string
// and keep their own state behind one slot each, which circkit_ctx_destroy releases.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/circkit.h"

hipStream_t ck_ctx_stream(circkit_ctx* c);
int ck_ctx_device(circkit_ctx* c);
// the ctx's complement table on the device: 256 bytes, bio 1.3.1 alphabets::dna (what the canonicalize kernels read)
const uint8_t* ck_ctx_complement(circkit_ctx* c);

// the ctx's last-error string = the formatted message (c may be null); returns `code`
int ck_fail(circkit_ctx* c, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int ck_ctx_fail(circkit_ctx* c, int code, const char* msg) { return ck_fail(c, code, "%s", msg); }

#define CK_HIP(c, call)                                                                             \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ck_fail(c, e_ == hipErrorOutOfMemory ? CIRCKIT_ERR_OOM : CIRCKIT_ERR_HIP,        \
                           "%s failed: %s", #call, hipGetErrorString(e_));                          \
    } while (0)

// One slot of state per unit: *slot is null until the unit puts its state there; circkit_ctx_destroy hands whatever it
// finds to the `release` the unit named.
enum ck_unit { CK_UNIT_ORFS, CK_UNIT_MONOMERIZE, CK_UNIT_UNIQ, CK_UNIT_UNIQ_COMPACT, CK_UNIT_WINDOWS, CK_UNIT_FASTA, CK_UNIT_FASTA_WRITE, CK_UNIT_SKETCH, CK_N_UNITS };
void** ck_ctx_slot(circkit_ctx* c, ck_unit unit, void (*release)(void*));
