// circkit_fasta.hip -- FASTA text on the device: the device form of the packer of fasta_host.cpp (include/circkit.h, "FASTA ->
// CSR on the device").  The routines are fasta_device.h's; here are the kernels around them and the ABI.
//
// A parse is five launches on the ctx stream, nothing waits and no workgroup waits for another:
//   fasta_bounds_kernel     the first byte that is no line end and the last '>' behind a '\n': two maxima over the text, from
//                           which every later kernel derives p0, limit and the format error (resolve_bounds)
//   fasta_summaries_kernel  summarize_tile over the tiles of TILE_BYTES
//   fasta_scan_kernel       one workgroup: the summaries become each tile's prefixes (state, records, bytes), SCAN_WG of them a
//                           round; then the totals, the refusals (capacity, overlap, format), offsets[0] and offsets[n_records]
//   fasta_apply_kernel      apply_tile over the tiles, unless the scan refused: payload, offsets, where the spans begin
//   fasta_spans_kernel      finish_spans per record, when spans were asked for
// The totals stay in device memory and are copied to page-locked memory behind the last kernel: circkit_fasta_parse_status waits
// for them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_ctx.h"
#include "ck_scan.h"
#include "fasta_device.h"
#include "fasta_host.h"

using ck_fasta::Prefix;
using ck_fasta::Span;
using ck_fasta::Summary;
using ck_fasta::Text;

static_assert(sizeof(Span) == sizeof(circkit_fasta_span) && sizeof(Span) == 16, "device span layout");

namespace {

constexpr uint32_t FASTA_GRID = 2048;                  // workgroups of the kernels over the text: 8 per CU, striding over the tiles
constexpr uint32_t SPANS_WG = 256, SPANS_MAX_GRID = 1u << 16;
constexpr int SCAN_WG = (int)ck_fasta::SCAN_WG;
// the totals of a parse, in device memory; the first two are the maxima of the bounds kernel (~position of the first byte that
// is no line end, so that 0 = none serves both)
enum { T_NOT_FIRST_BODY, T_LAST_CANDIDATE, T_RECORDS, T_BYTES, T_CONSUMED, T_REFUSED, T_STATE, T_WORDS };
enum { FLAG_FIRST = 1, FLAG_FINAL = 2 };

__device__ inline Text bounds_of(const uint8_t* text, uint64_t n, uint32_t flags, const uint64_t* totals, bool* error)
{
    return ck_fasta::resolve_bounds(text, n, ~totals[T_NOT_FIRST_BODY], totals[T_LAST_CANDIDATE], (flags & FLAG_FIRST) != 0, (flags & FLAG_FINAL) != 0,
                                    error);
}

__global__ __launch_bounds__(ck_fasta::WG) void fasta_bounds_kernel(const uint8_t* __restrict__ text, uint64_t n, uint64_t* __restrict__ totals)
{
    __shared__ uint64_t lo[ck_fasta::WG], hi[ck_fasta::WG];
    uint64_t first_body = ~0ull, last_candidate = 0;
    const uint64_t stride = 16ull * gridDim.x * ck_fasta::WG;
    for (uint64_t pos = 16ull * ((uint64_t)blockIdx.x * ck_fasta::WG + threadIdx.x); pos < n; pos += stride)
        ck_fasta::scan_bounds16(text, n, pos, &first_body, &last_candidate);
    lo[threadIdx.x] = first_body;
    hi[threadIdx.x] = last_candidate;
    __syncthreads();
    for (uint32_t d = ck_fasta::WG / 2; d; d >>= 1) {
        if (threadIdx.x < d) {
            if (lo[threadIdx.x + d] < lo[threadIdx.x]) lo[threadIdx.x] = lo[threadIdx.x + d];
            if (hi[threadIdx.x + d] > hi[threadIdx.x]) hi[threadIdx.x] = hi[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (lo[0] != ~0ull) atomicMax((unsigned long long*)&totals[T_NOT_FIRST_BODY], (unsigned long long)~lo[0]);
        if (hi[0]) atomicMax((unsigned long long*)&totals[T_LAST_CANDIDATE], (unsigned long long)hi[0]);
    }
}

__device__ inline void fill_lut(ck_fasta::Shared& S, const uint8_t* __restrict__ lut)
{
    for (uint32_t k = threadIdx.x; k < 256; k += ck_fasta::WG) S.lut[k] = lut[k];
    __syncthreads();
}

__global__ __launch_bounds__(ck_fasta::WG) void fasta_summaries_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t flags,
                                                                       const uint64_t* __restrict__ totals, const uint8_t* __restrict__ lut,
                                                                       Summary* __restrict__ summaries, uint64_t n_tiles)
{
    __shared__ ck_fasta::Shared S;
    fill_lut(S, lut);
    bool error;
    const Text T = bounds_of(text, n, flags, totals, &error);
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ck_fasta::summarize_tile(T, t, S, &summaries[t]);
}

// the scan of the state (ck_scan.h): the last event wins, ST_PASS hands the state on
struct StateOp {
    typedef uint32_t T;
    CK_DEV T identity() { return ck_fasta::ST_PASS; }
    CK_DEV T combine(T earlier, T later) { return ck_fasta::next_state(earlier, later); }
};

// One workgroup.  A round takes SCAN_WG summaries: the state in front of each tile first, which decides what the tile keeps,
// then the sums of records and bytes (one word: a round's records stay below 2^24, its bytes below 2^32).  The next round's
// summaries are loaded before this round's barriers.
__global__ __launch_bounds__(SCAN_WG) void fasta_scan_kernel(const Summary* __restrict__ summaries, uint64_t n_tiles, Prefix* __restrict__ prefix,
                                                             const uint8_t* text, uint64_t n, uint32_t flags, const uint8_t* out, uint64_t byte_capacity,
                                                             uint64_t record_capacity, uint64_t* __restrict__ offsets, uint64_t* __restrict__ totals)
{
    __shared__ uint32_t lds_state[SCAN_WG];
    __shared__ uint64_t lds_sum[SCAN_WG];
    bool error;
    const Text T = bounds_of(text, n, flags, totals, &error);
    uint64_t records = 0, bytes = 0;
    uint32_t state = ck_fasta::ST_SEQ;                 // in front of the text: no header is open
    const Summary none{ 0, 0, 0, 0 };
    Summary next = threadIdx.x < n_tiles ? summaries[threadIdx.x] : none;
    for (uint64_t b = 0; b < n_tiles; b += SCAN_WG) {
        const uint64_t idx = b + threadIdx.x;
        const Summary s = next;
        next = idx + SCAN_WG < n_tiles ? summaries[idx + SCAN_WG] : none;
        uint32_t last;
        const uint32_t in = ck_fasta::next_state(state, ck_scan::block_scan<SCAN_WG, StateOp>(threadIdx.x, s.kind, lds_state, &last));
        uint64_t total;
        const uint64_t before = ck_scan::block_scan<SCAN_WG, ck_scan::Add>(threadIdx.x, (uint64_t)s.starts << 32 | ck_fasta::tile_kept(s, in), lds_sum,
                                                                         &total);
        if (idx < n_tiles) prefix[idx] = Prefix{ records + (before >> 32), bytes + (before & 0xFFFFFFFFull), in };
        state = ck_fasta::next_state(state, last);
        records += total >> 32;
        bytes += total & 0xFFFFFFFFull;
    }
    if (threadIdx.x == 0) {
        uint32_t refused = error ? (uint32_t)ck_fasta::REFUSED_FORMAT : ck_fasta::verdict(records, bytes, record_capacity, byte_capacity, text, n, out);
        totals[T_RECORDS] = records;
        totals[T_BYTES] = bytes;
        totals[T_CONSUMED] = error ? 0 : T.limit;
        totals[T_REFUSED] = refused;
        totals[T_STATE] = state;
        offsets[0] = 0;
        if (!refused) offsets[records] = bytes;
    }
}

__global__ __launch_bounds__(ck_fasta::WG) void fasta_apply_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t flags,
                                                                   const uint64_t* __restrict__ totals, const uint8_t* __restrict__ lut,
                                                                   const Prefix* __restrict__ prefix, uint64_t n_tiles, uint8_t* __restrict__ out,
                                                                   uint64_t* __restrict__ offsets, Span* __restrict__ head, Span* __restrict__ raw)
{
    __shared__ ck_fasta::Shared S;
    fill_lut(S, lut);
    if (totals[T_REFUSED] || totals[T_RECORDS] == 0) return;      // the same for the whole grid
    bool error;
    ck_fasta::Apply A;
    A.T = bounds_of(text, n, flags, totals, &error);
    A.prefix = prefix;
    A.out = out; A.offsets = offsets; A.head = head; A.raw = raw;
    // the tiles that hold a byte of [p0, limit)
    const uint64_t t0 = A.T.p0 / ck_fasta::TILE_BYTES, t1 = (A.T.limit + ck_fasta::TILE_BYTES - 1) / ck_fasta::TILE_BYTES;
    for (uint64_t t = t0 + blockIdx.x; t < t1 && t < n_tiles; t += gridDim.x) ck_fasta::apply_tile(A, t, S);
}

__global__ __launch_bounds__(SPANS_WG) void fasta_spans_kernel(const uint8_t* __restrict__ text, uint64_t n, uint32_t flags,
                                                               const uint64_t* __restrict__ totals, Span* head, Span* raw)
{
    if (totals[T_REFUSED]) return;
    bool error;
    const Text T = bounds_of(text, n, flags, totals, &error);
    const uint64_t records = totals[T_RECORDS];
    const bool last_has_end = totals[T_STATE] == ck_fasta::ST_SEQ;
    const uint64_t stride = (uint64_t)gridDim.x * SPANS_WG;
    for (uint64_t r = (uint64_t)blockIdx.x * SPANS_WG + threadIdx.x; r < records; r += stride) ck_fasta::finish_spans(T, r, records, last_has_end, head, raw);
}

struct FastaState {
    ck_buf<uint8_t> d_lut;           // ckhost::normalize_lut(), copied when the slot is made
    ck_totals totals;                // [T_WORDS], made with the state
    uint64_t byte_capacity = 0, record_capacity = 0;       // of the most recent parse, for the status message
    bool any = false;
    ck_buf<Summary> d_summaries;
    ck_buf<Prefix> d_prefix;
    ck_buf<Span> d_spare;            // stands in for the one of d_head / d_raw that was not given
    // the staging of circkit_fasta_parse_text
    ck_buf<uint8_t> d_text, d_out;
    ck_buf<uint64_t> d_off;
    ck_buf<Span> d_head, d_raw;
};

int state(circkit_ctx* c, FastaState** out)
{
    FastaState* S = *out = ck_unit_state<FastaState>(c, CK_UNIT_FASTA);
    int rc;
    if (!S->d_lut) {
        if ((rc = S->d_lut.grow(c, 256))) return rc;
        hipError_t e = hipMemcpy(S->d_lut, ckhost::normalize_lut(), 256, hipMemcpyHostToDevice);
        if (e != hipSuccess) { S->d_lut.release(); CK_HIP(c, e); }
    }
    return ck_totals_make(c, &S->totals, T_WORDS);
}

// no text of n bytes holds more records than this: a record is at least ">\n", the last one at least ">"
uint64_t most_records(uint64_t n) { return (n + 1) / 2; }

int launch_parse(circkit_ctx* c, FastaState* S, const uint8_t* d_text, uint64_t n, int first_chunk, int final_chunk, uint8_t* d_out, uint64_t byte_capacity,
                 uint64_t* d_offsets, uint64_t record_capacity, Span* d_head, Span* d_raw)
{
    const uint64_t tiles = (n + ck_fasta::TILE_BYTES - 1) / ck_fasta::TILE_BYTES;
    int rc;
    if ((rc = S->d_summaries.grow(c, tiles))) return rc;
    if ((rc = S->d_prefix.grow(c, tiles))) return rc;
    if ((d_head != nullptr) != (d_raw != nullptr)) {
        const uint64_t most = most_records(n), spare = record_capacity < most ? record_capacity : most;
        if ((rc = S->d_spare.grow(c, spare))) return rc;
        if (!d_head) d_head = S->d_spare; else d_raw = S->d_spare;
    }
    const uint32_t flags = (first_chunk ? FLAG_FIRST : 0) | (final_chunk ? FLAG_FINAL : 0);
    const uint32_t grid = (uint32_t)(tiles < FASTA_GRID ? tiles : FASTA_GRID);
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, &S->totals, T_WORDS))) return rc;
    if (tiles) {
        hipLaunchKernelGGL(fasta_bounds_kernel, dim3(grid), dim3(ck_fasta::WG), 0, st, d_text, n, S->totals.d);
        hipLaunchKernelGGL(fasta_summaries_kernel, dim3(grid), dim3(ck_fasta::WG), 0, st, d_text, n, flags, (const uint64_t*)S->totals.d,
                           (const uint8_t*)S->d_lut, S->d_summaries, tiles);
    }
    hipLaunchKernelGGL(fasta_scan_kernel, dim3(1), dim3(SCAN_WG), 0, st, (const Summary*)S->d_summaries, tiles, S->d_prefix, d_text, n, flags,
                       (const uint8_t*)d_out, byte_capacity, record_capacity, d_offsets, S->totals.d);
    if (tiles) {
        hipLaunchKernelGGL(fasta_apply_kernel, dim3(grid), dim3(ck_fasta::WG), 0, st, d_text, n, flags, (const uint64_t*)S->totals.d,
                           (const uint8_t*)S->d_lut, (const Prefix*)S->d_prefix, tiles, d_out, d_offsets, d_head, d_raw);
        if (d_head) {
            const uint64_t most = most_records(n), upto = record_capacity < most ? record_capacity : most;
            const uint64_t want = (upto + SPANS_WG - 1) / SPANS_WG;
            if (want)
                hipLaunchKernelGGL(fasta_spans_kernel, dim3((uint32_t)(want < SPANS_MAX_GRID ? want : SPANS_MAX_GRID)), dim3(SPANS_WG), 0, st, d_text, n,
                                   flags, (const uint64_t*)S->totals.d, d_head, d_raw);
        }
    }
    CK_HIP(c, hipGetLastError());
    if ((rc = ck_totals_fetch(c, &S->totals, T_WORDS))) return rc;
    S->byte_capacity = byte_capacity;
    S->record_capacity = record_capacity;
    S->any = true;
    return CIRCKIT_OK;
}

// the verdict on totals the stream has delivered
int check_totals(circkit_ctx* c, const FastaState* S, const uint64_t* t)
{
    if (t[T_REFUSED] == ck_fasta::REFUSED_FORMAT)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "FASTA parse error: expected '>' at the start of the first record");
    if (t[T_REFUSED] == ck_fasta::REFUSED_CAPACITY)
        return ck_fail(c, CIRCKIT_ERR_OOM, "the text holds %llu records of %llu bytes, the buffers hold %llu records and %llu bytes: nothing was written",
                       (unsigned long long)t[T_RECORDS], (unsigned long long)t[T_BYTES], (unsigned long long)S->record_capacity,
                       (unsigned long long)S->byte_capacity);
    if (t[T_REFUSED]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_bytes overlaps the text: nothing was written");
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_fasta_parse_device(circkit_ctx* c, const uint8_t* d_text, uint64_t n_text, int first_chunk, int final_chunk, uint8_t* d_out_bytes,
                               uint64_t byte_capacity, uint64_t* d_out_offsets, uint64_t record_capacity, circkit_fasta_span* d_head,
                               circkit_fasta_span* d_raw)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if ((n_text && !d_text) || !d_out_offsets || (byte_capacity && !d_out_bytes)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_text > (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_text too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    FastaState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    return launch_parse(c, S, d_text, n_text, first_chunk, final_chunk, d_out_bytes, byte_capacity, d_out_offsets, record_capacity, (Span*)d_head,
                        (Span*)d_raw);
}

int circkit_fasta_parse_status(circkit_ctx* c, uint64_t* n_records, uint64_t* payload_bytes, uint64_t* consumed)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    FastaState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0 };
    const uint64_t* t = S->any ? S->totals.h : none;
    const bool format = t[T_REFUSED] == ck_fasta::REFUSED_FORMAT;
    if (n_records) *n_records = format ? 0 : t[T_RECORDS];
    if (payload_bytes) *payload_bytes = format ? 0 : t[T_BYTES];
    if (consumed) *consumed = t[T_CONSUMED];
    return check_totals(c, S, t);
}

int circkit_fasta_parse_text(circkit_ctx* c, const uint8_t* text, uint64_t n_text, int first_chunk, int final_chunk, uint8_t* out_bytes,
                             uint64_t byte_capacity, uint64_t* out_offsets, uint64_t record_capacity, circkit_fasta_span* head, circkit_fasta_span* raw,
                             uint64_t* n_records, uint64_t* payload_bytes, uint64_t* consumed)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if ((n_text && !text) || !out_offsets || (byte_capacity && !out_bytes)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_text > (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_text too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    FastaState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    // no text needs more than this, whatever the caller's buffers hold
    const uint64_t most = most_records(n_text);
    const uint64_t bytes_cap = byte_capacity < n_text ? byte_capacity : n_text, records_cap = record_capacity < most ? record_capacity : most;
    if ((rc = S->d_text.upload(c, text, n_text))) return rc;
    if ((rc = S->d_out.grow(c, bytes_cap))) return rc;
    if ((rc = S->d_off.grow(c, records_cap + 1))) return rc;
    if (head && (rc = S->d_head.grow(c, records_cap))) return rc;
    if (raw && (rc = S->d_raw.grow(c, records_cap))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = launch_parse(c, S, S->d_text, n_text, first_chunk, final_chunk, S->d_out, bytes_cap, S->d_off, records_cap, head ? S->d_head.p : nullptr,
                           raw ? S->d_raw.p : nullptr)))
        return rc;
    S->byte_capacity = byte_capacity;
    S->record_capacity = record_capacity;
    CK_HIP(c, hipStreamSynchronize(st));
    const uint64_t* t = S->totals.h;
    const bool format = t[T_REFUSED] == ck_fasta::REFUSED_FORMAT;
    const uint64_t R = format ? 0 : t[T_RECORDS], B = format ? 0 : t[T_BYTES];
    if (n_records) *n_records = R;
    if (payload_bytes) *payload_bytes = B;
    if (consumed) *consumed = t[T_CONSUMED];
    out_offsets[0] = 0;
    if (t[T_REFUSED]) return check_totals(c, S, t);
    if ((rc = S->d_out.download(c, out_bytes, B))) return rc;
    if (R && (rc = S->d_off.download(c, out_offsets, R + 1))) return rc;
    if ((rc = S->d_head.download(c, (Span*)head, R))) return rc;
    if ((rc = S->d_raw.download(c, (Span*)raw, R))) return rc;
    CK_HIP(c, hipStreamSynchronize(st));
    return CIRCKIT_OK;
}

}  // extern "C"
