/*
 * circkit.h -- C ABI of the MI355X (gfx950) drop-in for circkit's `canonicalize` / `uniq` hot path.
 *
 * The reference (Benjamin-Lee/circkit, Rust) has no FFI: the seam this library sits behind is the
 * lib-crate API plus the two closures the CLI hands to seq_io::parallel_fasta.  Each entry point below
 * names the reference interface it replaces (paths relative to the reference checkout); INTEGRATION.md
 * shows the `extern "C"` block a maintainer would add on the Rust side.
 *
 * Conventions
 *  - plain pointers and sizes only; caller allocates and owns every buffer; the library keeps no
 *    pointer after a call returns (device entry points: after the stream work completes).
 *  - return value 0 = CIRCKIT_OK, negative = error; no exceptions or panics cross the ABI;
 *    circkit_last_error(ctx) gives the message of the last failing call on that ctx.
 *  - one ctx per GPU, used by one host thread at a time; ctxs are independent (multi-GPU = one ctx,
 *    one process or thread, per device).
 *  - there is NO CPU fallback: every compute entry point runs the HIP kernels and fails with
 *    CIRCKIT_ERR_NO_DEVICE / CIRCKIT_ERR_HIP when it cannot.
 *  - CSR batches: bytes[offsets[i] .. offsets[i+1]) is record i; offsets has n_records + 1 entries,
 *    offsets[0] may be non-zero; records are what the reference's worker closure hands to
 *    circkit::canonicalize, i.e. already normalized (src/canonicalize.rs:24-29).  A record may be any
 *    byte string; records of pure ACGT take the 2-bit path, {-,A,C,G,N,T} the 4-bit path, everything
 *    else the byte-wide path (unsigned byte order, as the reference's slice comparison).
 */
#ifndef CIRCKIT_H
#define CIRCKIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIRCKIT_OK 0
#define CIRCKIT_ERR_INVALID_ARG (-1)
#define CIRCKIT_ERR_NO_DEVICE (-2)   /* no HIP device / device index out of range */
#define CIRCKIT_ERR_HIP (-3)         /* a HIP runtime call or kernel failed */
#define CIRCKIT_ERR_TOO_LONG (-4)    /* a record of 2^31 symbols or more (cyclic positions are 32-bit) */
#define CIRCKIT_ERR_OOM (-5)
#define CIRCKIT_ERR_NOT_ASCII (-6)   /* single-record API only: mirrors the reference's from_utf8().unwrap() panic */

typedef struct circkit_ctx circkit_ctx;

/* ---- context ---------------------------------------------------------------------------------- */
/* Replaces: nothing in the reference (it is a single CPU process); one ctx ~ one worker pool
 * (`--threads`, src/commands.rs:120-123) bound to one GPU. */
int circkit_ctx_create(int device, circkit_ctx** out);
int circkit_ctx_destroy(circkit_ctx* ctx);
const char* circkit_last_error(const circkit_ctx* ctx);
/* Launch all subsequent work of this ctx on `hip_stream` (a hipStream_t; NULL = HIP's default stream).
 * A fresh ctx launches on a private non-blocking stream; circkit_ctx_use_own_stream returns to it.
 * Switching ORDERS the streams: the new stream waits (on the device, through an event -- the host does not block) for
 * everything the ctx has queued on the stream it leaves, so un-synchronised batches on either side of a switch cannot
 * overlap in the ctx's lists, counters and table, and a call after the switch may read what a call before it wrote.
 * The stream being left must still exist.  Binding the stream that is already bound is free. */
int circkit_ctx_set_stream(circkit_ctx* ctx, void* hip_stream);
int circkit_ctx_use_own_stream(circkit_ctx* ctx);
/* Block until all work queued by this ctx has finished. */
int circkit_ctx_synchronize(circkit_ctx* ctx);
/* Milliseconds the canonicalize kernels of the most recent *_batch_device call took on the GPU
 * (hipEvent pair recorded on the launch stream around the kernels; synchronizes on the stop event). */
int circkit_ctx_last_kernel_ms(circkit_ctx* ctx, float* ms);

/* ---- batch, device resident (the hot path) ---------------------------------------------------- */
/* Replaces, for a whole batch of records: the worker-closure body `circkit::canonicalize(&normalized)`
 * (src/canonicalize.rs:29, src/uniq.rs:40) = lib/src/canonicalize.rs:54-63 (lmsr x2 + revcomp + select),
 * and, when d_out_xxh3 is given, `xxh3_64(canonicalized)` (src/uniq.rs:45).
 * All pointers are DEVICE pointers; the call only enqueues work on the ctx stream.
 *   d_bytes      payload; must be readable for total_bytes (= offsets[n_records]) bytes
 *   d_offsets    uint64[n_records + 1]
 *   d_out_bytes  nullable; canonical sequences, same offsets as the input
 *   d_out_index  nullable; uint32[n_records]: lmsr_index(s) when the forward strand wins, else
 *                lmsr_index(revcomp(lmsr(s))) -- the two indices the reference computes (:43, :56)
 *   d_out_strand nullable; uint8[n_records]: 0 = lmsr(s) returned, 1 = lmsr(revcomp) returned (:58-62)
 *   d_out_xxh3   nullable; uint64[n_records]: XXH3-64 (seed 0) of the canonical sequence
 * n_records must be < 2^30 and every record shorter than 2^31 bytes.  No alignment or padding is required of
 * d_bytes / d_out_bytes, and offsets[0] need not be 0.
 * The call enqueues EVERYTHING the batch needs: once the stream has run past it the outputs are complete, whichever
 * way the caller synchronises, and the next batch may be enqueued straight behind it.  Records too long for the
 * on-chip tiers (pure ACGT beyond ~640 kb, other alphabets beyond ~70-320 kb) are taken by the batch's last two
 * kernels in a ctx-owned global-memory scratch (256 MiB unless circkit_ctx_set_long_record_scratch says otherwise:
 * pure ACGT up to ~1 Gb, arbitrary bytes up to ~126 MB); a record beyond that is left untouched and counted by
 * circkit_ctx_batch_status. */
int circkit_canonicalize_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                      uint64_t n_records, uint8_t* d_out_bytes, uint32_t* d_out_index,
                                      uint8_t* d_out_strand, uint64_t* d_out_xxh3);

/* lmsr() for a whole batch: forward strand only (lib/src/canonicalize.rs:41-47); d_out_index[i] =
 * lmsr_index(record i) (lib/src/canonicalize.rs:5). */
int circkit_lmsr_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                              uint64_t n_records, uint8_t* d_out_bytes, uint32_t* d_out_index);
/* xxh3_64 (call site src/uniq.rs:45) of every record of a device-resident CSR batch. */
int circkit_xxh3_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                              uint64_t n_records, uint64_t* d_out_xxh3);

/* Waits for the most recent batch and returns the number of its records that could not be processed (longer than
 * the long-record scratch allows, or 2^31 symbols or more; they were left untouched): non-zero makes the status
 * CIRCKIT_ERR_TOO_LONG. */
int circkit_ctx_batch_status(circkit_ctx* ctx, uint32_t* n_unprocessed);
/* Size in bytes of the global-memory scratch the device entry points give to records beyond the on-chip tiers (a
 * record of n symbols needs ~0.25 n bytes when pure ACGT -- 0.38 n if its minimal 16-mer repeats --, ~1.13 n for
 * {-,A,C,G,N,T}, ~2.13 n otherwise).  The host-buffer entry points see the lengths and grow the scratch by
 * themselves.  Synchronizes. */
int circkit_ctx_set_long_record_scratch(circkit_ctx* ctx, uint64_t bytes);
/* Which build of the streaming kernel the most recent device batch selected, from that batch's own lengths: 1 = one
 * packed word per lane (records up to 1008 b), 2 = two words (a quarter or more of the records in 1009..2032 b),
 * 3 = neither (an eighth or more of the records longer; the per-record passes take everything).  Diagnostic: every
 * mode computes the same results (and the library launches a batch's kernels for the mode the batches before it reported,
 * so a change of kind costs one or two slower batches, never a wrong answer).  Synchronizes. */
int circkit_ctx_last_batch_mode(circkit_ctx* ctx, uint32_t* mode);

/* ---- batch, host buffers ---------------------------------------------------------------------- */
/* Same contract with HOST pointers: copies the batch into ctx-owned device buffers (grow-only), runs
 * circkit_canonicalize_batch_device, copies the requested outputs back and returns when they are complete.
 * Batches of 32 MB and more go through the device in up to sixteen parts: part k + 1 is copied in (on the ctx stream, behind
 * part k's kernels) while part k - 1 is copied out (on a stream of the ctx's own), so with page-locked buffers both
 * directions of the link are busy at once (1 GB of 1 kb records: 23-24 ms per call instead of 38; 64 MB: 2.0 ms; 16 MB: 0.8).
 * The offsets and the per-record outputs cross through page-locked staging of the ctx, whatever memory the caller's are in.
 * Buffers from circkit_host_alloc (page-locked) are copied by DMA; pageable memory goes through the runtime's
 * staging.  Streaming hosts overlap this call with their own parsing / writing (see circkit_cli.cpp).
 * offsets[0] must be 0. */
int circkit_canonicalize_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets,
                               uint64_t n_records, uint8_t* out_bytes, uint32_t* out_index,
                               uint8_t* out_strand, uint64_t* out_xxh3);

/* Page-locked host memory for batch buffers: with bytes / out_bytes allocated here the host-buffer entry points
 * copy by plain DMA instead of through the runtime's pageable staging.  Needs a HIP device (NULL otherwise). */
void* circkit_host_alloc(size_t bytes);
void circkit_host_free(void* p);

/* ---- single record: 1:1 mirror of the lib crate (lib/src/lib.rs:1,3) ------------------------------ */
/* pub fn lmsr_index(x: &[u8]) -> usize            lib/src/canonicalize.rs:5  */
int circkit_lmsr_index(circkit_ctx* ctx, const uint8_t* s, size_t n, size_t* out_index);
/* pub fn lmsr(s: &[u8]) -> Vec<u8>                lib/src/canonicalize.rs:41  (out has n bytes) */
int circkit_lmsr(circkit_ctx* ctx, const uint8_t* s, size_t n, uint8_t* out);
/* pub fn canonicalize(s: &[u8]) -> Vec<u8>        lib/src/canonicalize.rs:54  (out has n bytes) */
int circkit_canonicalize(circkit_ctx* ctx, const uint8_t* s, size_t n, uint8_t* out);
/* xxhash_rust::xxh3::xxh3_64(bytes)               call site src/uniq.rs:45 */
int circkit_xxh3_64(circkit_ctx* ctx, const uint8_t* s, size_t n, uint64_t* out_hash);

/* ---- uniq: first-seen resolution on the device ------------------------------------------------ */
/* Replaces the `seen: HashMap<u64, String, NoHash>` logic of src/uniq.rs:27,47-48,66: for every record
 * i, d_first_seen[i] = the smallest global index whose hash equals d_hash[i] (hash-only equality, as in
 * the reference); record i is kept iff d_first_seen[i] == base_index + i.
 * `base_index` is the global index of record 0 of this batch (multi-GPU sharding / streaming batches).
 * The table persists in the ctx across calls until circkit_uniq_reset, so batches (and hash sets
 * gathered from other GPUs) can be folded in one after another:
 *   circkit_uniq_insert_device   folds (hash, global index) pairs into the table
 *   circkit_uniq_lookup_device   reads the winner for each hash
 * A lookup (lookup_device, lookup_rows) of a hash that is not in the table answers ~0 (UINT64_MAX), which is no record's
 * index.  circkit_uniq_reset(expected_keys) sizes the table for that many DISTINCT keys (a power of two of at least 1024
 * slots, at most 70 % full); the hash ~0 has a slot of its own beside them and never takes one.  When more distinct keys
 * arrive than there are slots, the table fills completely, the records whose key found no slot are counted
 * (circkit_uniq_status) and every lookup of such a key answers ~0; the keys that did find a slot keep their right
 * answers.  circkit_uniq_reset clears the count with the table. */
int circkit_uniq_reset(circkit_ctx* ctx, uint64_t expected_keys);
int circkit_uniq_insert_device(circkit_ctx* ctx, const uint64_t* d_hash, uint64_t n, uint64_t base_index);
/* the same with an explicit global index per key: the keys a rank receives in the multi-GPU exchange (hash-range
 * partition, circkit_amd/uniq.py) are a subset of every other rank's shard, not a contiguous range */
int circkit_uniq_insert_pairs_device(circkit_ctx* ctx, const uint64_t* d_hash, const uint64_t* d_index, uint64_t n);
int circkit_uniq_lookup_device(circkit_ctx* ctx, const uint64_t* d_hash, uint64_t n, uint64_t* d_first_seen);
/* The device steps of the multi-GPU exchange (circkit_amd/uniq.py, exchange = "partition"; the reference is one process:
 * src/uniq.rs:27 has no counterpart).  The key space is cut into `world` (<= 64) ranges, a key belongs to rank
 * ((hash >> 20) & 0x7FFFFFFF) % world.
 *   partition    d_rows[n][2] = {hash, base_index + i} with the rows of one owner together, owners in rank order (what
 *                an all-to-all sends; any order inside an owner's group), d_counts[world] = rows per owner, d_slot[i] =
 *                row of record i.  n < 2^32 - 1.  d_rows -- here and in insert_rows / lookup_rows -- must be 16-byte
 *                aligned (a row is one 16-byte access).
 *   insert_rows  folds received rows into the table;  lookup_rows  d_answers[k] = smallest index seen for row k's hash
 *   gather       d_first_seen[i] = d_answers[d_slot[i]] (the answers come back in row order), d_keep[i] (nullable) =
 *                1 iff that is base_index + i */
int circkit_uniq_partition_device(circkit_ctx* ctx, const uint64_t* d_hash, uint64_t n, uint64_t base_index, uint32_t world,
                                  uint64_t* d_rows, uint64_t* d_counts, uint32_t* d_slot);
int circkit_uniq_insert_rows_device(circkit_ctx* ctx, const uint64_t* d_rows, uint64_t n);
int circkit_uniq_lookup_rows_device(circkit_ctx* ctx, const uint64_t* d_rows, uint64_t n, uint64_t* d_answers);
int circkit_uniq_gather_device(circkit_ctx* ctx, const uint64_t* d_answers, const uint32_t* d_slot, uint64_t n, uint64_t base_index,
                               uint64_t* d_first_seen, uint8_t* d_keep);
/* One shard in one call: reset (sized for n keys), insert with indices base_index .. base_index + n - 1, lookup, and
 * d_keep[i] (nullable, uint8) = 1 iff d_first_seen[i] == base_index + i -- the reference's per-record decision "emit,
 * or write a table row" (src/uniq.rs:47-62).  n < 2^32 - 1.  The table's contents are private to the call (it keeps
 * shard-local indices in a layout of its own): circkit_uniq_insert_* / _lookup_device refuse to touch it until the next
 * circkit_uniq_reset.  (Shards of 2^19 .. 21M keys are resolved in LDS-sized buckets with the table's memory as scratch --
 * same answers, no table contents at all afterwards; CIRCKIT_UNIQ_NO_BUCKETS=1 in the environment keeps the table path.) */
int circkit_uniq_resolve_device(circkit_ctx* ctx, const uint64_t* d_hash, uint64_t n, uint64_t base_index,
                                uint64_t* d_first_seen, uint8_t* d_keep);
/* reset / insert / lookup / resolve only enqueue work.  circkit_uniq_status waits for it and fails with CIRCKIT_ERR_OOM when
 * keys found no slot (more distinct keys than circkit_uniq_reset was told to expect); *n_overflowed (nullable) = how many inserted records (not distinct keys) that were, 0 without an overflow. */
int circkit_uniq_status(circkit_ctx* ctx, uint32_t* n_overflowed);

/* Host-buffer form for streaming hosts (the CLI's batch loop): folds this batch's hashes (global indices
 * base_index .. base_index + n - 1) into the ctx table -- created and grown on demand, earlier batches kept --
 * and returns first_seen[i] for the batch.  Synchronizes.  If growing the table fails half-way (a failed rehash), the
 * earlier batches are lost: this call and every later one return CIRCKIT_ERR_HIP until circkit_uniq_reset. */
int circkit_uniq_first_seen(circkit_ctx* ctx, const uint64_t* hash, uint64_t n, uint64_t base_index,
                            uint64_t* first_seen);

/* Replaces, for a whole batch, the writer side of src/uniq.rs:47-66 ("emit the record, or write a table row"): packs the
 * records that are the first with their hash back to back into a new CSR batch, which circkit_orfs_batch_device /
 * circkit_canonicalize_batch_device take as it is, and lists the others with their first occurrence -- the (id, duplicate_id)
 * rows of `--table`, as indices.  Device pointers; the call only enqueues work on the ctx stream.
 *   d_bytes        the payload to pack: the canonical bytes (`uniq -c`, :54-56) or the input's (:57-59); the call does not care
 *   d_first_seen   uint64[n_records], what circkit_uniq_resolve_device, circkit_uniq_lookup_device (streaming batches) or
 *                  circkit_uniq_gather_device (multi-GPU) wrote.  Record i is kept iff d_first_seen[i] == base_index + i; ANY
 *                  other value drops it, ~0 included.  ~0 is the answer for a key that found no slot in an overflowed table:
 *                  the caller owes a circkit_uniq_status before it trusts what was dropped.
 *   base_index     the global index of record 0 of this batch, as in the call that produced d_first_seen
 *   d_out_bytes    room for offsets[n_records] - offsets[0] bytes; must not overlap the input payload
 *   d_out_offsets  uint64[n_records + 1]: entries 0..m are written, d_out_offsets[0] = 0; m = the number of kept records
 *   d_out_src      uint64[n_records]: entries 0..m-1 are written, the input index of output record j, ascending
 *   d_dup_src      uint64[n_records] or null: entry k = the input index of dropped record number k, in input order (:67)
 *   d_dup_first    uint64[n_records] or null: entry k = that record's d_first_seen, a GLOBAL index: the first occurrence may
 *                  belong to an earlier batch (:66).  Entries 0..n_records-m-1 of the two are written, nothing beyond.
 * A zero-length record is a record: kept, it takes an entry of d_out_offsets and no bytes.  offsets[0] need not be 0; no
 * pointer needs any alignment.  A null required buffer with n_records > 0: INVALID_ARG; with n_records == 0, d_out_offsets[0]
 * = 0 is still written when that pointer is given.  Whether the output overlaps the payload depends on offsets that only the
 * device holds: the device checks it before anything is packed, writes no record and no index (d_out_offsets[0] = 0 aside),
 * and circkit_uniq_compact_status reports INVALID_ARG. */
int circkit_uniq_compact_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                const uint64_t* d_first_seen, uint64_t base_index,
                                uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src,
                                uint64_t* d_dup_src, uint64_t* d_dup_first);
/* Waits for the most recent uniq compact of this ctx (device or host form): *n_kept = its m, *kept_bytes = d_out_offsets[m].
 * CIRCKIT_ERR_INVALID_ARG when that compact refused its output buffer (see above); both totals are 0 then.  The totals are
 * this call's own: circkit_monomers_status keeps answering for the most recent monomer compact, and the other way round. */
int circkit_uniq_compact_status(circkit_ctx* ctx, uint64_t* n_kept, uint64_t* kept_bytes);
/* One shard of src/uniq.rs:27-66 with HOST buffers, on one stream: copy in, circkit_canonicalize_batch_device (the XXH3, and
 * the canonical bytes only when canonical_out), circkit_uniq_resolve_device with base 0, the compact of the canonical bytes
 * (canonical_out) or of the input, copy home; synchronizes.  Copied back: out_offsets[0..m], out_src[0..m), out_offsets[m]
 * bytes of out_bytes and, when given, first_seen[0..n_records) -- what the host writes the table rows from; *n_kept = m.
 * offsets[0] must be 0; n_records < 2^32 - 1 (resolve's limit; circkit_canonicalize_batch_device's own applies too).  A record
 * that the canonicalize batch leaves unprocessed (circkit_ctx_batch_status): CIRCKIT_ERR_TOO_LONG and nothing is returned; a
 * table overflow: the status of circkit_uniq_status.  The staging on the device is the ctx's and only grows.  As after
 * circkit_uniq_resolve_device, the ctx table is private to the call until the next circkit_uniq_reset. */
int circkit_uniq_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, int canonical_out,
                       uint8_t* out_bytes, uint64_t* out_offsets, uint64_t* out_src, uint64_t* first_seen, uint64_t* n_kept);

/* ---- circular ORFs (`circkit orfs`) --------------------------------------------------------------- */
/* One ORF as lib/src/orfs.rs:6-15 defines it (pub struct Orf), plus the strand it was found on.  start and stop are
 * positions on that strand (a reverse-strand ORF counts on revcomp(record), as the reference's RC list does);
 * length includes the start and stop codons. */
#define CIRCKIT_ORF_NO_STOP 0xFFFFFFFFu      /* stop: None */
#define CIRCKIT_ORF_MAX_CODONS 64
typedef struct circkit_orf {
    uint64_t length;
    uint32_t start;
    uint32_t stop;                           /* CIRCKIT_ORF_NO_STOP = None */
    uint32_t wraps;
    uint32_t strand;                         /* 0 forward, 1 reverse */
} circkit_orf;

/* The worker closure's settings (src/commands.rs:174-244 flags, src/orfs.rs:25-104 uses):
 *   start_codons / stop_codons  `--start-codons` / `--stop-codons` split at ','; a codon with a byte outside {ACGTN-}
 *                               (lower case included) is dropped: it never matches a normalized record.  The
 *                               batch entry points assume normalized records; on other bytes such a codon would
 *                               match where the reference's byte comparison does, and this library's does not.
 *                               Codons of another length never match either: leave them out.
 *   min_length .. require_stop  the retain() filter of src/orfs.rs:68-74: length - 3 >= min_length, a stop unless
 *                               !require_stop (`--no-stop-required`), min_wraps <= wraps <= max_wraps,
 *                               length / L >= min_ratio (an f64 division)
 *   strands                     bit 0 forward, bit 1 reverse (`--strand reverse` in the CLI still asks for both:
 *                               src/orfs.rs:79-103 always computes the forward list)
 *   mode                        0 = longest per stop, in longest_orfs' order (lib/src/orfs.rs:301-315: length, then
 *                               start % 3, then start, all descending); 1 = every ORF that passes the filter, in
 *                               find_orfs_with_indices' order (frame-major, start ascending) */
typedef struct circkit_orf_params {
    uint8_t start_codons[CIRCKIT_ORF_MAX_CODONS][3];
    uint32_t n_start_codons;
    uint8_t stop_codons[CIRCKIT_ORF_MAX_CODONS][3];
    uint32_t n_stop_codons;
    uint64_t min_length;
    double min_ratio;
    uint32_t min_wraps;
    uint32_t max_wraps;
    uint32_t require_stop;
    uint32_t strands;
    uint32_t mode;
} circkit_orf_params;

/* Replaces, for a whole batch of normalized records, the worker closure of src/orfs.rs:53-104:
 * start_stop_codon_indices_by_frame_naive (lib/src/orfs.rs:73) + find_orfs_with_indices (:149) + the filter +
 * longest_orfs (:301), once per strand.  Device pointers; the call only enqueues work on the ctx stream.
 *   d_orf_offsets  uint64[n_records + 1], always written in full: record i's ORFs are
 *                  d_orfs[d_orf_offsets[i] .. d_orf_offsets[i+1]), its forward ORFs before its reverse ones
 *   d_orfs         `capacity` descriptors; a record whose ORFs do not all fit below capacity is not written
 * Records of 0 or 1 symbols (a panic in the reference) have no ORFs; records of 2^32 symbols or more are not processed.
 * offsets[0] need not be 0. */
int circkit_orfs_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                              const circkit_orf_params* params, uint64_t* d_orf_offsets, circkit_orf* d_orfs,
                              uint64_t capacity);
/* Waits for the most recent ORF batch of this ctx (device or host form) and sets *total = its total number of ORFs
 * (d_orf_offsets[n_records]); CIRCKIT_ERR_OOM when that is more than the capacity it was given. */
int circkit_orfs_status(circkit_ctx* ctx, uint64_t* total);
/* The same with HOST buffers; synchronizes.  orf_offsets (n_records + 1) and *total are always written; when
 * *total > capacity nothing is written to orfs and the call returns CIRCKIT_ERR_OOM, so that the caller can grow its
 * buffer and call again.  offsets[0] must be 0. */
int circkit_orfs_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                       const circkit_orf_params* params, uint64_t* orf_offsets, circkit_orf* orfs, uint64_t capacity,
                       uint64_t* total);
/* pub fn find_orfs(seq: &str) -> Vec<Orf>         lib/src/orfs.rs:41
 * ATG / TAA,TAG,TGA, forward strand, no filter, find order; the bytes are compared as given (no normalization).
 * *count = the number of ORFs; CIRCKIT_ERR_OOM (and nothing in out) when it is more than capacity. */
int circkit_find_orfs(circkit_ctx* ctx, const uint8_t* s, size_t n, circkit_orf* out, size_t capacity, size_t* count);

/* ---- monomerize (`circkit monomerize`) ------------------------------------------------------------ */
#define CIRCKIT_MONOMER_NONE 0xFFFFFFFFu     /* end index: None (the record is no multimer under the settings) */
/* The Monomerizer's settings (lib/src/monomerize.rs:6-17; `--seed-length`, `--max-mismatch`, `--min-identity`,
 * `--sensitive` of src/commands.rs):
 *   seed_len       1..63 (MonomerizerBuilder::validate, lib/src/monomerize.rs:27-37); anything else: INVALID_ARG
 *   use_identity   0: an overlap may hold up to overlap_dist mismatches; 1: up to
 *                  ovl - floor(ovl * min_identity) of its ovl symbols (:70-76, the product in f64).  The two exclude
 *                  each other in the reference, hence the switch.
 *   min_identity   in [0, 1] when used (src/monomerize.rs:40-44); NaN and anything outside: INVALID_ARG
 *   sensitive      last_monomer_end_index_sensitive (:122) instead of last_monomer_end_index (:97) */
typedef struct circkit_monomerize_params {
    uint32_t seed_len;
    uint32_t use_identity;
    uint64_t overlap_dist;
    double min_identity;
    uint32_t sensitive;
} circkit_monomerize_params;

/* Replaces, for a whole batch of normalized records, the call of the worker closure of src/monomerize.rs:85-88:
 * Monomerizer::last_monomer_end_index / last_monomer_end_index_sensitive (lib/src/monomerize.rs:97, :122).
 * Device pointers; the call only enqueues work on the ctx stream.
 *   d_end   uint32[n_records]: record i's monomer is its first d_end[i] symbols; CIRCKIT_MONOMER_NONE = None
 * Nothing else is written (the monomer is a prefix of the input).  The worker's pre-check (a record shorter than the
 * seed or than --min-length) and the writer's filters are the caller's.  Records of 2^32 symbols or more are not
 * processed (NONE).  offsets[0] need not be 0.  The bytes are compared as given. */
int circkit_monomerize_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets,
                                    uint64_t n_records, const circkit_monomerize_params* params, uint32_t* d_end);
/* The same with HOST buffers; synchronizes.  offsets[0] must be 0; a record of 2^32 symbols or more:
 * CIRCKIT_ERR_TOO_LONG and nothing is computed. */
int circkit_monomerize_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                             const circkit_monomerize_params* params, uint32_t* end);
/* pub fn last_monomer_end_index(self, seq: &[u8]) -> Option<usize>             lib/src/monomerize.rs:97
 * pub fn last_monomer_end_index_sensitive(&self, seq: &[u8]) -> Option<usize>  lib/src/monomerize.rs:122
 * *found = 0 for None, and then *end = n, so that s[..*end] is Monomerizer::monomerize[_sensitive] (:138, :146). */
int circkit_monomer_end_index(circkit_ctx* ctx, const uint8_t* s, size_t n, const circkit_monomerize_params* params,
                              size_t* end, int* found);

/* The writer's filters (src/monomerize.rs:94-131; `--min-length`, `--max-length`, `--min-overlap`,
 * `--min-overlap-percent`, `-k` of src/commands.rs).  For a record of n symbols whose full_seq() holds f >= n bytes and
 * whose end index is idx:
 *   min_length / max_length   idx < min_length or idx > max_length: None (:97-103)
 *   min_overlap               f - idx < min_overlap: None (:106-112)
 *   min_overlap_percent       used iff use_min_overlap_percent: (f - idx) as f64 / idx as f64 < it: None (:115-125); one
 *                             IEEE division, so idx = 0 gives inf or NaN and a NaN threshold never rejects
 *   keep_all                  a record whose index is None is written whole instead of being dropped (:130-131) */
typedef struct circkit_monomer_filter {
    uint64_t min_length;            /* --min-length, 0 = none */
    uint64_t max_length;            /* --max-length, UINT64_MAX = none */
    uint64_t min_overlap;           /* --min-overlap, 0 = none */
    double   min_overlap_percent;   /* --min-overlap-percent, used iff use_min_overlap_percent */
    uint32_t use_min_overlap_percent;
    uint32_t keep_all;              /* -k */
} circkit_monomer_filter;

/* Replaces, for a whole batch, the writer closure of src/monomerize.rs:90-131 and the slicing `&full_seq[..end_idx]` (:135):
 * decides per record what the reference would write and packs the written monomers back to back into a new CSR batch,
 * which circkit_canonicalize_batch_device / circkit_uniq_* take as it is.  Device pointers; the call only enqueues work on
 * the ctx stream.
 *   d_end          the end indices of circkit_monomerize_batch_device; CIRCKIT_MONOMER_NONE or anything beyond its record:
 *                  None.  The worker's pre-check (:80) needs no step of its own: monomerize returns indices in
 *                  [seed_len, n - seed_len] only, so a record shorter than --min-length fails min_length.
 *   d_full_len     uint64[n_records] full_seq().len() per record (>= its normalized length), or null: the normalized length
 *   d_out_bytes    room for offsets[n_records] - offsets[0] bytes; must not overlap the input payload
 *   d_out_offsets  uint64[n_records + 1]: entries 0..m are written, d_out_offsets[0] = 0; m = the number of written records
 *   d_out_src      uint64[n_records]: entries 0..m-1 are written, the input index of output record j
 *   d_kept_end     uint32[n_records] or null: the index that survived the filters, or CIRCKIT_MONOMER_NONE
 * A record is written with its first idx bytes, or, under keep_all and without an index, whole.  offsets[0] need not be 0;
 * no pointer needs any alignment.  Null filter, or a null required buffer with n_records > 0: INVALID_ARG.  Whether the
 * output overlaps the payload depends on offsets that only the device holds: the device checks it before anything is
 * packed, writes no record, and circkit_monomers_status reports INVALID_ARG. */
int circkit_monomers_compact_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                    const uint32_t* d_end, const uint64_t* d_full_len, const circkit_monomer_filter* filter,
                                    uint8_t* d_out_bytes, uint64_t* d_out_offsets, uint64_t* d_out_src, uint32_t* d_kept_end);
/* Waits for the most recent compact of this ctx (device or host form): *n_kept = its m, *kept_bytes = d_out_offsets[m].
 * CIRCKIT_ERR_INVALID_ARG when that compact refused its output buffer (see above); both totals are 0 then. */
int circkit_monomers_status(circkit_ctx* ctx, uint64_t* n_kept, uint64_t* kept_bytes);
/* src/monomerize.rs:85-131 with HOST buffers: circkit_monomerize_batch_device and the compact on one stream; synchronizes.
 * offsets[0] must be 0; a record of 2^32 symbols or more: CIRCKIT_ERR_TOO_LONG and nothing is computed.  Copied back:
 * out_offsets[0..m], out_src[0..m), kept_end (when given) and out_offsets[m] bytes of out_bytes; *n_kept = m. */
int circkit_monomers_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                           const circkit_monomerize_params* params, const circkit_monomer_filter* filter,
                           const uint64_t* full_len, uint8_t* out_bytes, uint64_t* out_offsets, uint64_t* out_src,
                           uint32_t* kept_end, uint64_t* n_kept);

/* ---- cyclic windows (`circkit rotate` / `cat` / `decat`, reverse complements, ORF sequences) ------ */
/* One window: `length` bytes read cyclically from position `start` of record `record`, on the record or on its reverse
 * complement.  With n the record's length and S the record (strand 0) or revcomp(record) (strand 1:
 * S[j] = comp(s[n-1-j]), comp = bio 1.3.1's alphabets::dna complement, the table the canonicalize kernels use), the
 * window's bytes are S[(start + t) mod n] for t < length: Orf::seq_with_opts (lib/src/orfs.rs:19-35) for an ORF on either
 * strand, `&full_seq[idx..]` + `&full_seq[..idx]` of src/rotate.rs:42-43 with start = idx, the doubled record of
 * src/concatenate.rs:21-22 with length 2n. */
typedef struct circkit_window {
    uint64_t length;                         /* bytes to write; may exceed the record's length: the read goes round the record */
    uint32_t record;                         /* index into the batch */
    uint32_t start;                          /* first symbol ON THE STRAND NAMED; any value, taken mod the record's length */
    uint32_t strand;                         /* 0: the record; 1: revcomp(record) */
    uint32_t reserved;                       /* 0 */
} circkit_window;

/* Packs the windows' bytes back to back: out_bytes[out_offsets[k] .. out_offsets[k+1]) = window k.  Device pointers; the call
 * only enqueues work on the ctx stream.
 *   d_windows      n_windows windows (8-byte aligned); never written
 *   d_out_bytes    room for out_capacity bytes; must not overlap the input payload
 *   d_out_offsets  uint64[n_windows + 1], always written in full, d_out_offsets[0] = 0
 * A window on a record of 0 symbols writes no bytes whatever its length (the reference's cycle() over an empty slice yields
 * nothing).  A window with record >= n_records, strand > 1, reserved != 0, or on a record of 2^32 symbols or more is INVALID:
 * it is counted, written as an empty window and never dereferenced.  Lengths add up saturating: a total that does not fit 64
 * bits is UINT64_MAX, which no capacity holds.  When the total exceeds out_capacity, or [d_out_bytes, d_out_bytes + total)
 * overlaps the input payload (the offsets are the device's, so the device checks), no byte of d_out_bytes is written;
 * d_out_offsets is written all the same.  Null d_windows / d_out_offsets (or d_bytes / d_offsets with records, or d_out_bytes
 * with a capacity) and n_windows > 0: INVALID_ARG.  offsets[0] need not be 0; no pointer but d_windows needs any alignment. */
int circkit_windows_gather_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                  const circkit_window* d_windows, uint64_t n_windows, uint8_t* d_out_bytes,
                                  uint64_t out_capacity, uint64_t* d_out_offsets);
/* Waits for the most recent windows gather of this ctx (device or host form): *total_bytes = out_offsets[n_windows],
 * *n_invalid = its invalid windows.  CIRCKIT_ERR_OOM when the total exceeded the capacity, CIRCKIT_ERR_INVALID_ARG when the
 * output overlapped the payload or n_invalid != 0 (with n_invalid != 0 and nothing else wrong the valid windows ARE written). */
int circkit_windows_status(circkit_ctx* ctx, uint64_t* total_bytes, uint64_t* n_invalid);

/* One window per record, written on the device from the offsets (no host round trip); restates src/rotate.rs:20-43 and
 * src/concatenate.rs:21-22,45 for a record of n symbols:
 *   ROTATE_BASES    s = bases;  ROTATE_PERCENT  s = floor(n as f64 * percent) as i64 (Rust's `as`: saturating, NaN = 0)
 *                   idx = n - (s mod n) for s >= 0, |s| mod n otherwise (|i64::MIN| = 2^63); {n, i, idx mod n, 0}
 *                   bases == 0 / percent == 0.0 (-0.0 too): INVALID_ARG, "Rotation by 0 is not allowed", nothing enqueued
 *   CAT             {2n, i, 0, 0}      DECAT  {n / 2, i, 0, 0}      REVCOMP  {n, i, 0, 1}
 * A record of 0 symbols gets an empty window for every kind (the reference's `% 0` panics); a record of 2^32 symbols or more
 * a window the gather counts as invalid.  An unknown kind, or n_records > 2^32 - 1: INVALID_ARG. */
enum { CIRCKIT_WINDOWS_ROTATE_BASES, CIRCKIT_WINDOWS_ROTATE_PERCENT, CIRCKIT_WINDOWS_CAT, CIRCKIT_WINDOWS_DECAT, CIRCKIT_WINDOWS_REVCOMP };
int circkit_windows_of_records_device(circkit_ctx* ctx, const uint64_t* d_offsets, uint64_t n_records, uint32_t kind,
                                      int64_t bases, double percent, circkit_window* d_windows);
/* One window per ORF of a circkit_orfs_batch_device result: record = the record whose range of d_orf_offsets holds the ORF
 * (none: an invalid window), start / strand as the ORF's, length = orf.length - (include_stop ? 0 : 3), 0 below that
 * (`--include-stop`, src/orfs.rs:110-152).  The gather of these windows over the ORF batch's records is what `circkit orfs`
 * writes as sequence lines, in the list's order. */
int circkit_orfs_windows_device(circkit_ctx* ctx, const uint64_t* d_orf_offsets, const circkit_orf* d_orfs, uint64_t n_records,
                                uint64_t n_orfs, int include_stop, circkit_window* d_windows);
/* circkit_windows_gather_device with HOST buffers; synchronizes.  out_offsets (n_windows + 1) and *total are always written;
 * when *total > out_capacity nothing is written to out_bytes and the call returns CIRCKIT_ERR_OOM, so that the caller can
 * grow its buffer and call again.  Invalid windows: CIRCKIT_ERR_INVALID_ARG after the valid ones were written.  offsets[0]
 * must be 0 and the offsets must not decrease. */
int circkit_windows_gather(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                           const circkit_window* windows, uint64_t n_windows, uint8_t* out_bytes, uint64_t out_capacity,
                           uint64_t* out_offsets, uint64_t* total);

/* ---- proteins of cyclic windows ------------------------------------------------------------------ */
/* With L the bytes circkit_windows_gather_device writes for a window (0 on an empty record and for an invalid window) and S,
 * n as above, the window's protein has L / 3 residues (one or two trailing symbols are ignored); residue t is
 *   aa[16 c(S[(start + 3t) mod n]) + 4 c(S[(start + 3t + 1) mod n]) + c(S[(start + 3t + 2) mod n])]
 * with c('T') = 0, c('C') = 1, c('A') = 2, c('G') = 3: the order of NCBI's genetic-code strings.  A codon with any other byte
 * (N, '-', lower case: batches are normalized) is `unknown`.  On a record of 1 or 2 symbols a codon reads a symbol more than
 * once.  With first_as_m, residue 0 of every window whose first codon is three ACGT symbols is 'M' whatever the table says (an
 * alternative start codon reads as methionine); an unknown first codon stays `unknown`.  The protein of window k is the plain
 * translation of the bytes circkit_windows_gather_device writes for window k. */
typedef struct circkit_translate_params {
    uint8_t aa[64];                          /* residue per codon, index 16*c0 + 4*c1 + c2 with T,C,A,G = 0..3 (an NCBI "AAs" line) */
    uint8_t unknown;                         /* residue of a codon with a byte outside ACGT, e.g. 'X' */
    uint8_t first_as_m;                      /* 0 / 1 */
    uint8_t reserved[6];                     /* 0 */
} circkit_translate_params;

/* Packs the windows' proteins back to back: out_aa[out_offsets[k] .. out_offsets[k+1]) = window k's residues.  The contract is
 * circkit_windows_gather_device's with residues in place of bytes: device pointers, the call only enqueues work;
 * d_out_offsets[0 .. n_windows] is always written in full and the sums saturate; when the total exceeds out_capacity, or
 * [d_out_aa, d_out_aa + total) overlaps the input payload (the device decides), no byte of d_out_aa is written; invalid windows
 * are counted and empty, their neighbours are written; the null-pointer and alignment rules are the gather's.  Null params,
 * first_as_m > 1 or a reserved byte in use: INVALID_ARG, nothing enqueued.  With the stop codon in the window
 * (circkit_orfs_windows_device, include_stop) the protein ends in the table's stop residue. */
int circkit_windows_translate_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                     const circkit_window* d_windows, uint64_t n_windows, const circkit_translate_params* params,
                                     uint8_t* d_out_aa, uint64_t out_capacity, uint64_t* d_out_offsets);
/* Waits for the most recent translate of this ctx (device or host form): *total_residues = out_offsets[n_windows], *n_invalid =
 * its invalid windows; the return values are circkit_windows_status's.  The totals are the translate's own: this call and
 * circkit_windows_status each answer for the most recent call of their kind, whatever ran in between. */
int circkit_translate_status(circkit_ctx* ctx, uint64_t* total_residues, uint64_t* n_invalid);
/* circkit_windows_translate_device with HOST buffers; synchronizes.  out_offsets (n_windows + 1) and *total are always written;
 * when *total > out_capacity nothing is written to out_aa and the call returns CIRCKIT_ERR_OOM, so that the caller can grow
 * its buffer and call again.  Invalid windows: CIRCKIT_ERR_INVALID_ARG after the valid ones were written.  offsets[0] must be
 * 0 and the offsets must not decrease. */
int circkit_windows_translate(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                              const circkit_window* windows, uint64_t n_windows, const circkit_translate_params* params,
                              uint8_t* out_aa, uint64_t out_capacity, uint64_t* out_offsets, uint64_t* total);

/* ---- sketches of circular records ---------------------------------------------------------------- */
/* Nothing in the reference is replaced: its roadmap names `cluster` and `prealign` as the next commands, and both need a cheap
 * similarity between circular records that depends neither on where a record was cut nor on the strand read.  This section is
 * the definition.  A record of n symbols (n < 2^31) has, when n >= k, the n cyclic k-mers of the symbols (p + i) mod n,
 * i = 0..k-1, one per start p; when n < k it has none.  A k-mer is VALID when its k bytes are all of A C G T (upper case: the
 * batches are normalized; lower case, N, '-' and anything else make it invalid, and it is skipped).  f = the k-mer packed to 2k
 * bits with A, C, G, T = 0..3, first symbol most significant; r = the same packing of its reverse complement; c = min(f, r);
 *   h = fmix64(c ^ seed),  fmix64 = MurmurHash3's finalizer:  h ^= h >> 33; h *= 0xff51afd7ed558ccd; h ^= h >> 33;
 *                                                             h *= 0xc4ceb9fe1a85ec53; h ^= h >> 33
 * The record's sketch is a row of s = 1 << log2_bins words: row[b] = the minimum h over the valid k-mers with
 * h >> (64 - log2_bins) == b, CIRCKIT_SKETCH_EMPTY where there is none (the one k-mer in 2^64 whose h is 2^64 - 1 is, by
 * definition, indistinguishable from an empty bin).  n_kmers = the number of valid k-mers, that one included.  The row is a
 * function of the multiset of canonical cyclic k-mers: bit-identical for every rotation of the record, for its reverse
 * complement, and (n >= k) for the record twice in a row. */
typedef struct circkit_sketch_params {
    uint32_t k;                              /* 4 .. 32 */
    uint32_t log2_bins;                      /* 4 .. 10: 16 .. 1024 bins */
    uint64_t seed;
    uint32_t reserved[2];                    /* 0 */
} circkit_sketch_params;
#define CIRCKIT_SKETCH_EMPTY 0xFFFFFFFFFFFFFFFFull

/* The sketch of every record of a batch (no counterpart in the reference: its roadmap's `cluster` / `prealign`).  Device
 * pointers; the call only enqueues work on the ctx stream.  offsets[0] need not be 0; d_bytes needs no alignment.
 *   d_out_sketch   uint64[n_records << log2_bins], 8-byte aligned: row i = record i's; every row is written in full, the rows
 *                  of records with n < k (all EMPTY) included
 *   d_out_n_kmers  uint32[n_records] or null: the valid k-mers of every record
 * A record of 2^31 symbols or more is not dereferenced: it gets an all-EMPTY row and count 0, and is counted
 * (circkit_sketch_status).  The outputs must not overlap the inputs: against the offsets and each other the host checks
 * (INVALID_ARG); the payload's extent is the device's, and keeping the outputs off it is the caller's contract.  k, log2_bins
 * out of range, reserved != 0, null params or null buffers with records: INVALID_ARG, nothing enqueued.  n_records == 0 is
 * valid.  The result is bit-identical from run to run. */
int circkit_sketch_batch_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                const circkit_sketch_params* params, uint64_t* d_out_sketch, uint32_t* d_out_n_kmers);
/* Waits for the most recent sketch of this ctx (device or host form; no counterpart in the reference, roadmap `cluster`):
 * *n_valid_kmers_total = the valid k-mers of all records, *n_unprocessed = the records of 2^31 symbols or more;
 * CIRCKIT_ERR_TOO_LONG when n_unprocessed != 0.  The totals are the sketch's own: this call answers for the most recent sketch
 * whatever other unit ran in between, as circkit_fasta_write_status does for its kind. */
int circkit_sketch_status(circkit_ctx* ctx, uint64_t* n_valid_kmers_total, uint32_t* n_unprocessed);
/* Compares rows of two sketch arrays over a list of pairs (no counterpart in the reference, roadmap `cluster` / `prealign`).
 * Pair p = (i, j) = d_pairs[2p], d_pairs[2p + 1]: i indexes d_sketch_a (n_a rows), j indexes d_sketch_b (n_b rows), rows of
 * 1 << log2_bins words; the two arrays may be the same pointer.  d_out[2p] = match = the bins with A[b] == B[b] != EMPTY,
 * d_out[2p + 1] = filled = the bins with A[b] != EMPTY or B[b] != EMPTY.  match / filled is the one-permutation-hashing estimate
 * of the Jaccard index of the two k-mer sets; the caller divides.  A pair with i >= n_a or j >= n_b is INVALID: it is written
 * as (0, 0) and counted, and nothing it names is dereferenced.  Device pointers (the sketches 8-byte, the pairs and d_out
 * 4-byte aligned); the call only enqueues.  log2_bins out of range, null buffers with pairs, or d_out overlapping an input:
 * INVALID_ARG, nothing enqueued.  n_pairs == 0 is valid. */
int circkit_sketch_compare_device(circkit_ctx* ctx, const uint64_t* d_sketch_a, uint64_t n_a, const uint64_t* d_sketch_b,
                                  uint64_t n_b, uint32_t log2_bins, const uint32_t* d_pairs, uint64_t n_pairs, uint32_t* d_out);
/* Waits for the most recent compare of this ctx (device or host form; roadmap `cluster`, nothing replaced): *n_invalid = its
 * invalid pairs; CIRCKIT_ERR_INVALID_ARG when there was any, after the valid pairs were written. */
int circkit_sketch_compare_status(circkit_ctx* ctx, uint64_t* n_invalid);
/* circkit_sketch_batch_device with HOST buffers (roadmap `cluster`, nothing replaced): copies the batch in, sketches, copies the
 * rows and counts (out_n_kmers may be null) home and synchronizes.  offsets[0] must be 0 and the offsets must not decrease; a
 * record of 2^31 symbols or more is refused from the offsets alone, before anything is read: CIRCKIT_ERR_TOO_LONG, nothing
 * computed.  The staging is the ctx's and only grows. */
int circkit_sketch_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                         const circkit_sketch_params* params, uint64_t* out_sketch, uint32_t* out_n_kmers);
/* circkit_sketch_compare_device with HOST buffers (roadmap `cluster`, nothing replaced): copies the rows and pairs in, compares,
 * copies the results home and synchronizes; invalid pairs: CIRCKIT_ERR_INVALID_ARG after the valid ones were written. */
int circkit_sketch_compare(circkit_ctx* ctx, const uint64_t* sketch_a, uint64_t n_a, const uint64_t* sketch_b, uint64_t n_b,
                           uint32_t log2_bins, const uint32_t* pairs, uint64_t n_pairs, uint32_t* out);

/* ---- clusters of circular records ---------------------------------------------------------------- */
/* Nothing in the reference is replaced: `cluster` is the first open item of its roadmap.  This section is the definition: which
 * pairs of records are worth a compare (LSH banding over the sketch rows), and which records belong together once the pairs are
 * scored (single linkage).
 * BAND KEYS.  Band b of record i covers bins [b * band_bins, (b + 1) * band_bins) of its row.  If any of them is
 * CIRCKIT_SKETCH_EMPTY the band has no key.  Otherwise x = (b + 1) * 0x9e3779b97f4a7c15 mod 2^64, then for each bin in order
 * x = fmix64(x ^ bin) (the fmix64 of the sketch section); the key is x, except that x == 2^64 - 1 means "no key", as the empty
 * bin does.
 * CANDIDATES.  rep(key) = the smallest record index that has that key in any band.  Record i proposes, band by band in
 * ascending b, the pair (rep(key(i, b)), i) when rep < i and no earlier band of the same record proposed the same rep (the first
 * band wins).  So a pair is (smaller, larger), a record proposes at most n_bands pairs, and the members of a bucket are paired
 * with its first holder, not with each other.  The definition is in terms of equal KEYS: a collision of two keys behaves the
 * same in every implementation.
 * LINKING.  Over n_pairs pairs with the (match, filled) the compare wrote for each: a pair with an index >= n_records is
 * INVALID (counted, skipped, nothing dereferenced); a pair with i == j is skipped before its scores are read and is neither
 * invalid nor linked; any other pair LINKS when filled >= min_filled and ((uint64)match << 16) >= (uint64)min_similarity_q16 *
 * filled.  labels[i] = the smallest record index in i's connected component of the linked pairs (single linkage); the order of
 * the pairs does not reach the result.  Record i is a representative iff labels[i] == i, so the labels are a valid
 * d_first_seen for circkit_uniq_compact_device with base_index = 0. */
typedef struct circkit_cluster_params {
    uint32_t n_bands;                        /* 1 .. 64 */
    uint32_t band_bins;                      /* 1 .. 16; n_bands * band_bins <= 1 << log2_bins */
    uint32_t min_similarity_q16;             /* 0 .. 65536: a pair links iff (match << 16) >= min_similarity_q16 * filled ... */
    uint32_t min_filled;                     /* >= 1: ... and filled >= min_filled */
    uint32_t reserved[2];                    /* 0 */
} circkit_cluster_params;

/* The candidate pairs of the rows d_sketch (uint64[n_records << log2_bins], what circkit_sketch_batch_device wrote) as a CSR by
 * the later record (no counterpart in the reference: its roadmap's `cluster`).  Device pointers; the call only enqueues work on
 * the ctx stream.
 *   d_pair_offsets  uint64[n_records + 1], 8-byte aligned, always written in full ([0] = 0 also with n_records == 0)
 *   d_pairs         uint32[2 * capacity], 4-byte aligned: d_pairs[2p], d_pairs[2p + 1] = pair p; record i's pairs lie in
 *                   [d_pair_offsets[i], d_pair_offsets[i + 1]) in band order -- the layout circkit_sketch_compare_device takes
 * As with circkit_orfs_batch_device, a record whose pairs do not all lie below `capacity` is not written; the offsets and the
 * total are exact all the same, and circkit_cluster_candidates_status returns CIRCKIT_ERR_OOM.  capacity = n_records * n_bands
 * always suffices.  The smallest record with an equal key comes from circkit_uniq_resolve_device over the n_records * n_bands
 * keys: as after that call, the ctx's uniq table is private to this one until the next circkit_uniq_reset.  Parameters out of
 * range, reserved != 0, n_bands * band_bins > 1 << log2_bins, log2_bins outside 4 .. 10, null buffers (d_pairs may be null with
 * capacity 0), n_records >= 2^32 or n_records * n_bands >= 2^32 - 1, or an output that overlaps the sketch or the other output:
 * INVALID_ARG, nothing enqueued, buffers and earlier totals unchanged.  The result is bit-identical from run to run. */
int circkit_cluster_candidates_device(circkit_ctx* ctx, const uint64_t* d_sketch, uint64_t n_records, uint32_t log2_bins,
                                      const circkit_cluster_params* params, uint64_t* d_pair_offsets, uint32_t* d_pairs,
                                      uint64_t capacity);
/* Waits for the most recent candidates call of this ctx (roadmap `cluster`, nothing replaced): *total_pairs =
 * d_pair_offsets[n_records]; CIRCKIT_ERR_OOM when that is more than the capacity it was given, or when keys of the call's own
 * resolve found no slot (their bands proposed nothing).  The total and that count are this call's own, taken behind its resolve:
 * whatever other unit ran in between, a later use of the ctx's uniq table and its circkit_uniq_status included. */
int circkit_cluster_candidates_status(circkit_ctx* ctx, uint64_t* total_pairs);
/* Single linkage over scored pairs (roadmap `cluster`, nothing replaced): d_pairs and d_scores are uint32[2 * n_pairs] (what the
 * candidates and circkit_sketch_compare_device wrote, or any other list: either orientation, duplicates and self pairs are
 * fine), d_labels uint64[n_records], 8-byte aligned, always written in full.  n_bands and band_bins of the parameters are
 * checked and not used.  Device pointers; the call only enqueues.  Parameters out of range, n_records >= 2^32, null buffers
 * with work, or d_labels overlapping an input: INVALID_ARG, nothing enqueued.  n_records == 0 and n_pairs == 0 are valid.  The
 * labels are bit-identical from run to run. */
int circkit_cluster_link_device(circkit_ctx* ctx, uint64_t n_records, const uint32_t* d_pairs, const uint32_t* d_scores,
                                uint64_t n_pairs, const circkit_cluster_params* params, uint64_t* d_labels);
/* Waits for the most recent link of this ctx (device or host form; roadmap `cluster`, nothing replaced): *n_clusters = the
 * records with labels[i] == i, *n_linked = the pairs that passed the threshold, *n_invalid = the invalid pairs;
 * CIRCKIT_ERR_INVALID_ARG when there was any, after the valid pairs were applied.  The totals are the link's own. */
int circkit_cluster_link_status(circkit_ctx* ctx, uint64_t* n_clusters, uint64_t* n_linked, uint64_t* n_invalid);
/* The whole chain with HOST buffers on one stream (roadmap `cluster`, nothing replaced): copy in, circkit_sketch_batch_device,
 * the candidates with capacity n_records * n_bands, one wait for their number, circkit_sketch_compare_device, the link, copy the
 * labels (uint64[n_records]) home, synchronize; *n_clusters (nullable) = the number of representatives.  offsets[0] must be 0
 * and the offsets must not decrease; a record of 2^31 symbols or more is refused from the offsets alone: CIRCKIT_ERR_TOO_LONG,
 * nothing computed.  The staging is the ctx's and only grows; the ctx's uniq table is private to the call until the next
 * circkit_uniq_reset. */
int circkit_cluster_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                          const circkit_sketch_params* sketch, const circkit_cluster_params* params, uint64_t* labels,
                          uint64_t* n_clusters);

/* ---- pre-alignment of circular records ----------------------------------------------------------- */
/* Nothing in the reference is replaced: `prealign` is the second open item of its roadmap.  The members of a cluster were each
 * cut at an arbitrary position and read on an arbitrary strand; this section is the definition of the rotation and strand that
 * put record b onto record a, from the k-mers their sketches share.
 * ANCHORS.  For a record of n symbols and the parameters of the sketch section (k, log2_bins, seed), with `row` its sketch:
 * anchor[b] = 2 * p + o, where p is the SMALLEST start whose valid cyclic k-mer has h == row[b], and o = (r < f) for the k-mer at
 * that start: its reverse complement packs smaller, so the canonical form is the other strand's (a palindromic k-mer has o = 0).
 * anchor[b] = CIRCKIT_ANCHOR_NONE where row[b] is CIRCKIT_SKETCH_EMPTY.  p < 2^31, so the word fits 32 bits.  The row is
 * rotation-invariant and the anchors are not: that is the point.
 * VOTES.  For a pair (a, b) with lengths n_a, n_b (0 < n_b < 2^31), every bin with row_a[bin] == row_b[bin] != EMPTY and both
 * anchors != NONE is a MATCH, and votes: with pa, oa, pb, ob unpacked from the two anchors, s = oa ^ ob; if s == 1,
 * pb = (n_b - pb - k) mod n_b (the same k-mer's start on revcomp(b)); start = (pb - pa) mod n_b, the mathematical (non-negative)
 * modulus -- pa may exceed n_b; the vote is the 32-bit key (s << 31) | start.
 * RESULT.  matches = the number of matching bins; votes = the largest number of equal keys, ties going to the SMALLEST key
 * (strand 0 before strand 1, then the smaller start).  If votes >= min_votes the pair is ALIGNED and its window is
 * {length n_b, record b, start, strand s, 0}: the circkit_window whose bytes put b's counterpart of a's position 0 first.
 * Otherwise the window is the identity {n_b, b, 0, 0, 0}.  The scores (votes, matches) are always written.  A pair with
 * a >= n_records or b >= n_records is INVALID: window {0, b, 0, 0, 0}, scores (0, 0), counted, and nothing it names is read.
 * n_b == 0 gives {0, b, 0, 0, 0}; n_b >= 2^31 the identity window with that length; in both cases no bin votes (votes = 0) and
 * matches is counted all the same.  A pair (i, i) is aligned at (0, 0) with votes == matches.  Anchors enter arithmetic only:
 * nothing is dereferenced through them, and start < n_b holds by construction for any anchor values. */
typedef struct circkit_prealign_params {
    uint32_t k;                              /* 4 .. 32: the k the anchors were made with */
    uint32_t log2_bins;                      /* 4 .. 10: of the rows and the anchors */
    uint32_t min_votes;                      /* >= 1: a pair is aligned iff its votes reach this */
    uint32_t reserved;                       /* 0 */
} circkit_prealign_params;
#define CIRCKIT_ANCHOR_NONE 0xFFFFFFFFu

/* circkit_sketch_batch_device that writes the anchors too (no counterpart in the reference: its roadmap's `prealign`): the
 * contract is that call's, and the rows and counts are bit-identical to what it writes.  In addition
 *   d_out_anchors  uint32[n_records << log2_bins], 4-byte aligned, written in full: CIRCKIT_ANCHOR_NONE for all-EMPTY rows and
 *                  for records that are not processed
 * A null d_out_anchors with records, or one that overlaps the offsets or another output: INVALID_ARG, nothing enqueued.
 * circkit_sketch_status answers for this call as for "the most recent sketch".  Bit-identical from run to run. */
int circkit_sketch_anchors_device(circkit_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                  const circkit_sketch_params* params, uint64_t* d_out_sketch, uint32_t* d_out_n_kmers,
                                  uint32_t* d_out_anchors);
/* The window and scores of every pair (roadmap `prealign`, nothing replaced).  d_sketch and d_anchors are what
 * circkit_sketch_anchors_device wrote for the batch whose offsets are d_offsets (uint64[n_records + 1]; only the lengths are
 * read); d_pairs is uint32[2 * n_pairs] in the compare's layout: the candidates, circkit_prealign_pairs_of_labels_device or any
 * other list.  d_windows: n_pairs circkit_window, 8-byte aligned, what circkit_windows_gather_device takes; d_scores:
 * uint32[2 * n_pairs], (votes, matches).  Device pointers; the call only enqueues.  k or log2_bins out of the sketch's range,
 * min_votes == 0, reserved != 0, null buffers with work, n_records >= 2^32, or an output overlapping an input or the other
 * output: INVALID_ARG, nothing enqueued, buffers and earlier totals unchanged.  n_pairs == 0 and n_records == 0 are valid. */
int circkit_prealign_pairs_device(circkit_ctx* ctx, const uint64_t* d_sketch, const uint32_t* d_anchors, const uint64_t* d_offsets,
                                  uint64_t n_records, const circkit_prealign_params* params, const uint32_t* d_pairs,
                                  uint64_t n_pairs, circkit_window* d_windows, uint32_t* d_scores);
/* Waits for the most recent pairs call of this ctx (device or host form; roadmap `prealign`, nothing replaced): *n_aligned = its
 * aligned pairs, *n_invalid = its invalid pairs; CIRCKIT_ERR_INVALID_ARG when there was any, after the valid pairs were written.
 * The totals are the call's own, whatever other unit ran in between. */
int circkit_prealign_status(circkit_ctx* ctx, uint64_t* n_aligned, uint64_t* n_invalid);
/* Pair i = (d_labels[i], i) for the labels of circkit_cluster_link_device (roadmap `prealign`, nothing replaced): every record
 * against its representative, d_pairs uint32[2 * n_records].  A label of 2^32 or more is written as 0xFFFFFFFF, which the pairs
 * call counts as invalid.  Device pointers (d_labels 8-byte, d_pairs 4-byte aligned); only enqueues.  Null buffers with records,
 * n_records >= 2^32 or overlapping buffers: INVALID_ARG, nothing enqueued. */
int circkit_prealign_pairs_of_labels_device(circkit_ctx* ctx, const uint64_t* d_labels, uint64_t n_records, uint32_t* d_pairs);
/* The chain with HOST buffers on one stream (roadmap `prealign`, nothing replaced): copy in, circkit_sketch_anchors_device,
 * circkit_prealign_pairs_device with (sketch->k, sketch->log2_bins, min_votes), copy the windows (n_pairs) and scores
 * (uint32[2 * n_pairs]) home, synchronize.  offsets[0] must be 0 and the offsets must not decrease; a record of 2^31 symbols or
 * more is refused from the offsets alone: CIRCKIT_ERR_TOO_LONG, nothing computed.  Invalid pairs: CIRCKIT_ERR_INVALID_ARG after
 * the valid ones were written.  The staging is the ctx's and only grows. */
int circkit_prealign_batch(circkit_ctx* ctx, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
                           const circkit_sketch_params* sketch, const uint32_t* pairs, uint64_t n_pairs, uint32_t min_votes,
                           circkit_window* windows, uint32_t* scores);

/* ---- edit distance of record pairs --------------------------------------------------------------- */
/* Nothing in the reference is replaced: this is the first linear tool behind `prealign`, which puts two records into one frame.
 * BATCHES AND PAIRS.  Two CSR batches, A (d_bytes_a, d_offsets_a, n_a records) and B (likewise); they may be the same pointers.
 * offsets[0] need not be 0 and the payloads need no alignment.  Pair p = (i, j) = d_pairs[2p], d_pairs[2p + 1], in the compare's
 * layout: i indexes A, j indexes B; x = A[i] with n_x symbols, y = B[j] with n_y symbols.
 * SYMBOLS are bytes, equal iff their bytes are equal: N equals N, a differs from A, there is no wildcard, 0x00 and 0xFF are legal.
 * RESULT.  lev(x, y) is the Levenshtein distance with unit costs for substitution, insertion and deletion.  With
 * W = params.max_distance: distance = lev(x, y) if lev(x, y) <= W, CIRCKIT_DISTANCE_OVER otherwise.  This depends on no band
 * geometry: any correct bounded algorithm gives the same bits.  Part of the contract: |n_x - n_y| > W gives OVER and no byte of
 * either record is read; an empty record against one of n <= W symbols gives n; a pair (i, i) on one batch gives 0.  A pair with
 * i >= n_a or j >= n_b, or in which either record has 2^31 symbols or more, is INVALID: distance OVER, scores (0, 0), counted, and
 * nothing it names is read.
 * SCORES.  For a valid pair, with L = max(n_x, n_y): (L - distance, L) when the distance is within W, (0, L) when OVER.  This is
 * the (match, filled) layout circkit_cluster_link_device takes: a pair links iff filled >= min_filled and
 * ((L - d) << 16) >= min_similarity_q16 * L, that is identity 1 - d / L of at least the threshold, and d <= W. */
typedef struct circkit_distance_params {
    uint32_t max_distance;                   /* W: 0 .. CIRCKIT_DISTANCE_MAX */
    uint32_t reserved[3];                    /* 0 */
} circkit_distance_params;
#define CIRCKIT_DISTANCE_MAX 255u
#define CIRCKIT_DISTANCE_OVER 0xFFFFFFFFu

/* The distance and scores of every pair (no counterpart in the reference).  Device pointers; the call only enqueues on the ctx
 * stream.  d_offsets_a / d_offsets_b: uint64[n + 1], 8-byte aligned; d_pairs: uint32[2 * n_pairs]; d_out_distance:
 * uint32[n_pairs], nullable; d_out_scores: uint32[2 * n_pairs], nullable; all 4-byte aligned.  Both outputs null with pairs,
 * max_distance out of range, reserved != 0, null inputs with work, n_a or n_b >= 2^32, or an output overlapping the offsets, the
 * pairs or the other output: INVALID_ARG, nothing enqueued, buffers and earlier totals unchanged.  Keeping the outputs off the
 * payloads is the caller's contract, as in the sketch unit.  n_pairs == 0 is valid.  Bit-identical from run to run. */
int circkit_distance_pairs_device(circkit_ctx* ctx, const uint8_t* d_bytes_a, const uint64_t* d_offsets_a, uint64_t n_a,
                                  const uint8_t* d_bytes_b, const uint64_t* d_offsets_b, uint64_t n_b,
                                  const circkit_distance_params* params, const uint32_t* d_pairs, uint64_t n_pairs,
                                  uint32_t* d_out_distance, uint32_t* d_out_scores);
/* Waits for the most recent pairs call of this ctx (device or host form): *n_within = its pairs with a distance of at most W,
 * *n_invalid = its invalid pairs; CIRCKIT_ERR_INVALID_ARG when there was any, after the valid pairs were written.  The totals are
 * the call's own, whatever other unit ran in between. */
int circkit_distance_status(circkit_ctx* ctx, uint64_t* n_within, uint64_t* n_invalid);
/* The same with HOST buffers on one stream: copy in (once when A and B are the same pointers), the pairs call, copy the outputs
 * that are not null home, synchronize.  offsets[0] must be 0 and the offsets must not decrease; a record of 2^31 symbols or more
 * is refused from the offsets alone: CIRCKIT_ERR_TOO_LONG, nothing computed.  Invalid pairs: CIRCKIT_ERR_INVALID_ARG after the
 * valid ones were written.  The staging is the ctx's and only grows. */
int circkit_distance_pairs(circkit_ctx* ctx, const uint8_t* bytes_a, const uint64_t* offsets_a, uint64_t n_a,
                           const uint8_t* bytes_b, const uint64_t* offsets_b, uint64_t n_b, const circkit_distance_params* params,
                           const uint32_t* pairs, uint64_t n_pairs, uint32_t* out_distance, uint32_t* out_scores);

/* ---- FASTA -> CSR packer (host logic, no GPU) --------------------------------------------------- */
/* Replaces seq_io 0.3.2's fasta::Reader record boundaries + the normalize step of the worker closure
 * (src/canonicalize.rs:14-27, src/uniq.rs:24-38).  Parses the complete records of text[0, n): header span,
 * raw sequence span (RefRecord::seq(): interior line breaks kept, final one dropped) and the normalized
 * bytes in CSR layout (padded with 64 zero bytes).  first_chunk: skip leading blank lines and require '>';
 * final_chunk = 0: the last record may be cut by the chunk end, parsing stops at its start and *consumed
 * says where to resume.  Returns CIRCKIT_ERR_INVALID_ARG on a format error (message: circkit_fasta_error). */
typedef struct circkit_fasta_batch circkit_fasta_batch;
int circkit_fasta_parse(const uint8_t* text, size_t n, int first_chunk, int final_chunk, circkit_fasta_batch** out,
                        size_t* consumed);
const char* circkit_fasta_error(const circkit_fasta_batch* b);
uint64_t circkit_fasta_n_records(const circkit_fasta_batch* b);
const uint8_t* circkit_fasta_bytes(const circkit_fasta_batch* b);
const uint64_t* circkit_fasta_offsets(const circkit_fasta_batch* b);
int circkit_fasta_record(const circkit_fasta_batch* b, uint64_t i, size_t* head_off, size_t* head_len, size_t* raw_off,
                         size_t* raw_len);
void circkit_fasta_free(circkit_fasta_batch* b);

/* ---- FASTA -> CSR on the device ------------------------------------------------------------------ */
/* The device form of circkit_fasta_parse (ckhost::parse_chunk, fasta_host.cpp): the same records, spans, normalized bytes and
 * `consumed` for the same text and flags, byte for byte -- seq_io 0.3.2's record boundaries and needletail 0.5.1
 * normalize(_, false) (src/canonicalize.rs:14-27, src/uniq.rs:24-38).  One difference: without first_chunk the text's first byte
 * starts a record whatever it is, and a '\n' there is part of no header end (the host routine reads in front of the text then). */
typedef struct circkit_fasta_span { uint64_t off, len; } circkit_fasta_span;   /* into the text */

/* Parses d_text[0, n_text) into the CSR batch d_out_bytes / d_out_offsets, which circkit_canonicalize_batch_device,
 * circkit_monomerize_batch_device, circkit_orfs_batch_device and the other batch calls take as it is.  Device pointers; the call
 * only enqueues work on the ctx stream.  No pointer needs any alignment; the text is never written; n_text up to 2^40, 0 is valid.
 *   d_out_offsets   uint64[record_capacity + 1]; [0] = 0 is always written
 *   d_head, d_raw   circkit_fasta_span[record_capacity] each, or null: header and raw sequence span of every record, as
 *                   circkit_fasta_record reports them
 * The counts are always produced (circkit_fasta_parse_status).  When the records exceed record_capacity or the payload exceeds
 * byte_capacity (CIRCKIT_ERR_OOM with the true counts), when [d_out_bytes, d_out_bytes + payload) overlaps the text (the device
 * decides; CIRCKIT_ERR_INVALID_ARG) or on the format error (CIRCKIT_ERR_INVALID_ARG, the host routine's message, zero records),
 * no payload byte, no offset beyond [0] and no span is written: grow the buffers and call again.  byte_capacity = n_text and
 * record_capacity = (n_text + 1) / 2 always suffice.  Nothing is written outside [d_out_bytes, d_out_bytes + payload),
 * d_out_offsets[0 .. n_records] and the first n_records spans. */
int circkit_fasta_parse_device(circkit_ctx* ctx, const uint8_t* d_text, uint64_t n_text, int first_chunk, int final_chunk,
                               uint8_t* d_out_bytes, uint64_t byte_capacity, uint64_t* d_out_offsets, uint64_t record_capacity,
                               circkit_fasta_span* d_head, circkit_fasta_span* d_raw);
/* Waits for the most recent device parse of this ctx (device or host form): its records, payload bytes and `consumed`, and its
 * verdict as described above. */
int circkit_fasta_parse_status(circkit_ctx* ctx, uint64_t* n_records, uint64_t* payload_bytes, uint64_t* consumed);
/* circkit_fasta_parse_device with HOST buffers: copies the text in, parses, copies the batch home and synchronizes.  The counts
 * are always written; on CIRCKIT_ERR_OOM nothing but they and out_offsets[0] is.  The staging is the ctx's and only grows. */
int circkit_fasta_parse_text(circkit_ctx* ctx, const uint8_t* text, uint64_t n_text, int first_chunk, int final_chunk,
                             uint8_t* out_bytes, uint64_t byte_capacity, uint64_t* out_offsets, uint64_t record_capacity,
                             circkit_fasta_span* head, circkit_fasta_span* raw, uint64_t* n_records, uint64_t* payload_bytes,
                             uint64_t* consumed);

/* ---- FASTA text from the device ------------------------------------------------------------------ */
/* The inverse of circkit_fasta_parse_device: what every command of the reference writes (src/canonicalize.rs:33-37,
 * src/uniq.rs:50-61, src/orfs.rs:111-122,144-152, src/rotate.rs, src/concatenate.rs, src/monomerize.rs), packed back to back.
 * Output record k =  '>'  head_k  label_k  '\n'  body_k  '\n'
 *   i_k     = d_labels ? d_labels[k].record : k                       (must be < n_src)
 *   h_k     = d_src ? d_src[i_k] : i_k                                (must be < n_heads; with d_src null, n_src == n_heads)
 *   head_k  = d_text[d_head[h_k].off .. + d_head[h_k].len)
 *   label_k = d_labels ? (strand ? "_RC_ORF" : "_ORF") + decimal(d_labels[k].start) : nothing     (src/orfs.rs:113-114,146-147)
 *   body_k  = d_body ? d_body[d_body_offsets[k] .. d_body_offsets[k+1]) : d_text[d_raw[h_k].off .. + d_raw[h_k].len)
 * exactly one of d_body (with d_body_offsets, uint64[n_out + 1]) and d_raw is given.  d_head / d_raw are the spans of
 * circkit_fasta_parse_device, d_src the d_out_src of either compact, d_labels what circkit_orfs_windows_device writes (the
 * array that cuts the ORF sequences or proteins labels them; its `length` is not read).  The number is the u32 in plain decimal,
 * 1 to 10 digits; there is no line wrapping.
 * Device pointers; the call only enqueues work on the ctx stream.  No pointer but the 8-byte arrays needs any alignment; neither
 * the text nor the body is written.  d_out_offsets (uint64[n_out + 1], [0] = 0) is always written in full; lengths add up
 * saturating (a total that does not fit 64 bits is UINT64_MAX, which no capacity holds).  When the total exceeds out_capacity,
 * or [d_out_text, d_out_text + total) overlaps the text or the body payload d_body[d_body_offsets[0] .. d_body_offsets[n_out])
 * (the offsets are the device's, so the device decides), no byte of d_out_text is written.  A record is INVALID when
 * i_k >= n_src, h_k >= n_heads, its head or raw span does not lie in [0, n_text) (off > n_text or len > n_text - off), its label
 * has strand > 1 or reserved != 0, or its body range decreases or leaves the payload: it is counted and written as zero bytes,
 * and nothing it names is dereferenced.  Null / non-null combinations that make no sense (both or neither of d_body and d_raw,
 * d_body without d_body_offsets, null d_out_offsets, null d_out_text with a capacity, null d_src with n_src != n_heads), or
 * n_text > 2^40, or n_heads, n_src or n_out >= 2^40: INVALID_ARG, nothing enqueued.  n_out == 0 is valid. */
int circkit_fasta_write_device(circkit_ctx* ctx, const uint8_t* d_text, uint64_t n_text, const circkit_fasta_span* d_head,
                               const circkit_fasta_span* d_raw, uint64_t n_heads, const uint64_t* d_src, uint64_t n_src,
                               const circkit_window* d_labels, const uint8_t* d_body, const uint64_t* d_body_offsets,
                               uint64_t n_out, uint8_t* d_out_text, uint64_t out_capacity, uint64_t* d_out_offsets);
/* Waits for the most recent write of this ctx (device or host form): *total_bytes = out_offsets[n_out], *n_invalid = its invalid
 * records.  CIRCKIT_ERR_OOM when the total exceeded the capacity, CIRCKIT_ERR_INVALID_ARG when the output overlapped an input
 * or n_invalid != 0 (with n_invalid != 0 and nothing else wrong the valid records ARE written).  The totals are the write's
 * own: circkit_fasta_parse_status, circkit_windows_status and circkit_translate_status answer for their kind as before. */
int circkit_fasta_write_status(circkit_ctx* ctx, uint64_t* total_bytes, uint64_t* n_invalid);
/* circkit_fasta_write_device with HOST buffers; synchronizes.  out_offsets (n_out + 1) and *total are always written; when
 * *total > out_capacity nothing is written to out_text and the call returns CIRCKIT_ERR_OOM, so that the caller can grow its
 * buffer and call again.  Invalid records: CIRCKIT_ERR_INVALID_ARG after the valid ones were written.  body_offsets must not
 * decrease; body[0 .. body_offsets[n_out]) is copied in.  The staging is the ctx's and only grows. */
int circkit_fasta_write_text(circkit_ctx* ctx, const uint8_t* text, uint64_t n_text, const circkit_fasta_span* head,
                             const circkit_fasta_span* raw, uint64_t n_heads, const uint64_t* src, uint64_t n_src,
                             const circkit_window* labels, const uint8_t* body, const uint64_t* body_offsets, uint64_t n_out,
                             uint8_t* out_text, uint64_t out_capacity, uint64_t* out_offsets, uint64_t* total);

/* ---- synthetic input on the device (bench / tests) ------------------------------ */
/* Fills d_bytes[0..n_bases) with uniform ACGT from the counter-based generator keyed by
 * (seed, first_base + i) -- the same bytes oracle/ck_oracle_synth_fill produces on the host. */
int circkit_synth_fill_device(circkit_ctx* ctx, uint64_t seed, uint64_t first_base, uint64_t n_bases,
                              uint8_t* d_bytes);
/* d_offsets[i] = base + i * record_len for i in 0..n_records (inclusive). */
int circkit_fixed_offsets_device(circkit_ctx* ctx, uint64_t base, uint64_t record_len, uint64_t n_records,
                                 uint64_t* d_offsets);

/* Measurement helper, no counterpart in the reference (the roofline is quoted against what this very box
 * copies): enqueues ONE plain device-to-device copy of `bytes` bytes (rounded down to a multiple of 16; both buffers
 * 16-byte aligned) on the ctx stream.  variant 0..3 = copy kernels of different shapes (16 B per lane; 4 / 8 / 4 / 2 loads
 * in flight per lane over 2048 / 2048 / 8192 / 65536 workgroups), 4 = hipMemcpyAsync.  bench.py times each and reports the
 * best as roofline.copy_ceiling_gbps. */
int circkit_bench_copy_device(circkit_ctx* ctx, const void* d_src, void* d_dst, uint64_t bytes, uint32_t variant);

/* ---- host-side normalisation used by the packer ------------------------------------------------ */
/* needletail::sequence::normalize(seq, false)      call sites src/canonicalize.rs:24, src/uniq.rs:35
 * Host logic of the CSR packer (strips line breaks while it computes offsets); returns the new length,
 * sets *changed to 0 when the reference would have returned None. */
size_t circkit_normalize(const uint8_t* s, size_t n, uint8_t* out, int* changed);

const char* circkit_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CIRCKIT_H */
