// ck_compact_launch.h -- what a unit other than circkit_monomerize.hip may ask of the compact's scan / apply / gather kernels
// (internal; not part of the C ABI).
//
// The kernels live in circkit_monomerize.hip and know a record only by the word w[i] = ck_compact::WRITTEN | its written bytes
// (0: not written).  Who fills w decides what a compact means: the monomer compact applies the writer's filters
// (ck_compact::decide), the uniq compact compares first_seen with the record's own index (ck_compact::decide_uniq).  The scratch
// (w, the tile sums, the written records' source positions) is the ctx's, shared by every caller: all of it is used in
// stream order.  The TOTALS are the caller's, so that one unit's status call never answers for another unit's compact.
#pragma once
#include <stdint.h>

#include "ck_ctx.h"

// the words of a unit's most recent compact (a ck_totals of ck_ctx.h): written by the scan on the device, copied to pinned memory
// behind the gather
enum { CK_COMPACT_RECORDS, CK_COMPACT_BYTES, CK_COMPACT_OVERLAP, CK_COMPACT_WORDS };

// The scratch sized for n records (grow only); *d_w = the n words the caller's decide kernel fills on the ctx stream.
int ck_compact_reserve(circkit_ctx* c, uint64_t n, uint64_t** d_w);

// Tile sums, scan of sums (with the totals, out_offsets[0] and the refusal of an output that overlaps the payload), apply,
// gather, and the copy of the totals into T->h (T is made at the first launch): enqueued on the ctx stream behind the kernel
// that filled the reserved w; nothing waits.  Record i with w[i] = 0 is dropped; dropped record number k (in input order) writes
// d_dup_src[k] = i and d_dup_first[k] = d_dup_val[i], each of the two where the pointer is given (d_dup_val is read only for
// d_dup_first).
int ck_compact_launch(circkit_ctx* c, ck_totals* T, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                      uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src, uint64_t* d_dup_src, uint64_t* d_dup_first,
                      const uint64_t* d_dup_val);
