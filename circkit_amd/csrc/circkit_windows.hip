// circkit_windows.hip -- cyclic windows of a device batch: the windows section of include/circkit.h.
//
// A gather is five steps on the ctx stream, nothing waits:
//   windows_lengths_kernel     one lane per window: out_offsets[k + 1] = the bytes window k writes (window_gather.h
//                              effective_length: 0 for an invalid window and on an empty record), invalid windows counted
//   windows_tile_sums_kernel   the sum of each tile of WSCAN_TILE lengths
//   windows_scan_sums_kernel   one workgroup: the tile sums become exclusive; then the total, its comparison with the
//                              capacity and the refusal of an output that overlaps the payload
//   windows_apply_kernel       out_offsets in place: the lengths become the offsets
//   windows_gather_kernel      window_gather.h gather_tile over the output tiles, unless the scan refused the gather
// The three scan kernels are ck_scan.h's bodies with WSCAN_WG, WSCAN_ITEMS and the saturating sum (ck_scan::SatAdd), so
// out_offsets never decreases whatever lengths the windows name.  The totals stay in device memory and are
// copied to pinned memory behind the gather: circkit_windows_status waits and reads them.
// A translate (window_translate.h) is the same five steps with its own first and last: windows_residues_kernel counts residues
// (a third of the bytes, rounded down), the three scan kernels run as they are, windows_translate_kernel runs translate_tile
// over the output tiles.  Its totals are its own, so circkit_windows_status and circkit_translate_status each answer for the
// most recent call of their kind whatever ran in between.
// windows_of_records_kernel and orfs_windows_kernel write the window lists of rotate / cat / decat / revcomp and of an ORF
// batch from what the device already holds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "ck_scan.h"
#include "window_gather.h"
#include "window_translate.h"

using ck_windows::Window;

static_assert(sizeof(Window) == sizeof(circkit_window) && sizeof(Window) == 24, "device window layout");
static_assert(sizeof(circkit_translate_params) == 72, "translate params layout");
static_assert((int)ck_windows::KIND_ROTATE_BASES == CIRCKIT_WINDOWS_ROTATE_BASES && (int)ck_windows::KIND_ROTATE_PERCENT == CIRCKIT_WINDOWS_ROTATE_PERCENT &&
              (int)ck_windows::KIND_CAT == CIRCKIT_WINDOWS_CAT && (int)ck_windows::KIND_DECAT == CIRCKIT_WINDOWS_DECAT &&
              (int)ck_windows::KIND_REVCOMP == CIRCKIT_WINDOWS_REVCOMP, "window kinds");

namespace {

constexpr int WIN_WG = 256;                            // lengths, of_records, orfs_windows: one lane per item
constexpr int WSCAN_WG = 256, WSCAN_ITEMS = 8, WSCAN_TILE = WSCAN_WG * WSCAN_ITEMS;      // windows per scan tile: 2048
constexpr uint32_t WIN_MAX_GRID = 1u << 20;            // the lanes stride over the items beyond this many workgroups
constexpr uint32_t GATHER_GRID = 2048;                 // workgroups of the gather: 8 per CU, striding over the output tiles
enum { T_TOTAL, T_INVALID, T_REFUSED, T_WORDS };       // the totals of a gather, in device memory
enum { REFUSED_CAPACITY = 1, REFUSED_OVERLAP = 2 };

__global__ __launch_bounds__(WIN_WG) void windows_lengths_kernel(const uint64_t* __restrict__ offsets, uint64_t n_records,
                                                                 const Window* __restrict__ windows, uint64_t m,
                                                                 uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ totals)
{
    const uint64_t stride = (uint64_t)gridDim.x * WIN_WG;
    for (uint64_t k = (uint64_t)blockIdx.x * WIN_WG + threadIdx.x; k < m; k += stride) {
        bool invalid;
        out_offsets[k + 1] = ck_windows::effective_length(windows[k], offsets, n_records, &invalid);
        if (invalid) atomicAdd((unsigned long long*)&totals[T_INVALID], 1ull);
    }
}

__global__ __launch_bounds__(WIN_WG) void windows_residues_kernel(const uint64_t* __restrict__ offsets, uint64_t n_records,
                                                                  const Window* __restrict__ windows, uint64_t m,
                                                                  uint64_t* __restrict__ out_offsets, uint64_t* __restrict__ totals)
{
    const uint64_t stride = (uint64_t)gridDim.x * WIN_WG;
    for (uint64_t k = (uint64_t)blockIdx.x * WIN_WG + threadIdx.x; k < m; k += stride) {
        bool invalid;
        out_offsets[k + 1] = ck_translate::residue_length(windows[k], offsets, n_records, &invalid);
        if (invalid) atomicAdd((unsigned long long*)&totals[T_INVALID], 1ull);
    }
}

__global__ __launch_bounds__(WSCAN_WG) void windows_tile_sums_kernel(const uint64_t* __restrict__ len, uint64_t m, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[WSCAN_WG];
    const uint64_t total = ck_scan::tile_sum<WSCAN_WG, WSCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, len, m, [](uint64_t w) { return w; }, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the tile sums become exclusive, WSCAN_WG of them at a time; then the total, out_offsets[0], and the two
// refusals: a total beyond the capacity, and an output [out, out + total) that overlaps the input payload.
__global__ __launch_bounds__(WSCAN_WG) void windows_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles, const uint8_t* bytes,
                                                                     const uint64_t* __restrict__ offsets, uint64_t n_records, const uint8_t* out,
                                                                     uint64_t capacity, uint64_t* __restrict__ out_offsets,
                                                                     uint64_t* __restrict__ totals)
{
    __shared__ uint64_t lds[WSCAN_WG];
    const uint64_t total = ck_scan::sums_exclusive<WSCAN_WG, ck_scan::SatAdd>(threadIdx.x, sums, n_tiles, lds);
    if (threadIdx.x == 0) {
        uint64_t refused = total > capacity || total == ~0ull ? REFUSED_CAPACITY : 0;
        if (!refused && total && out && n_records) {
            const uint64_t p0 = offsets[0], p1 = offsets[n_records];
            const uintptr_t in_lo = (uintptr_t)bytes + p0, in_hi = (uintptr_t)bytes + p1, out_lo = (uintptr_t)out, out_hi = out_lo + total;
            if (p1 > p0 && out_lo < in_hi && in_lo < out_hi) refused = REFUSED_OVERLAP;
        }
        totals[T_TOTAL] = total;
        totals[T_REFUSED] = refused;
        if (out_offsets) out_offsets[0] = 0;
    }
}

// out_offsets[k + 1]: window k's length becomes where it ends
__global__ __launch_bounds__(WSCAN_WG) void windows_apply_kernel(uint64_t* __restrict__ ends, uint64_t m, const uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[WSCAN_WG];
    ck_scan::apply_ends<WSCAN_WG, WSCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, ends, m, sums, lds);
}

__global__ __launch_bounds__(64 * ck_windows::GATHER_WAVES) void windows_gather_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                                                        uint64_t n_records, const Window* __restrict__ windows, uint64_t m,
                                                                                        const uint64_t* __restrict__ out_offsets,
                                                                                        const uint64_t* __restrict__ totals, const uint8_t* __restrict__ comp,
                                                                                        uint8_t* __restrict__ out)
{
    __shared__ uint8_t comp_lds[256];
    for (uint32_t k = threadIdx.x; k < 256; k += 64 * ck_windows::GATHER_WAVES) comp_lds[k] = comp[k];
    __syncthreads();
    if (totals[T_REFUSED]) return;                    // the same for the whole grid
    ck_windows::Gather G;
    G.bytes = bytes; G.offsets = offsets;
    G.p0 = offsets[0]; G.p1 = offsets[n_records];
    G.windows = windows; G.out_offsets = out_offsets;
    G.m = m; G.B = totals[T_TOTAL];
    G.comp = comp_lds;
    G.out = out;
    if (G.B == 0) return;
    const uint64_t n_gran = (((uint64_t)(uintptr_t)out & 15u) + G.B + 15) / 16;
    const uint64_t n_tiles = (n_gran + ck_windows::TILE_GRANULES - 1) / ck_windows::TILE_GRANULES;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ck_windows::gather_tile(G, t);
}

__global__ __launch_bounds__(64 * ck_translate::TRANSLATE_WAVES) void windows_translate_kernel(
    const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n_records, const Window* __restrict__ windows, uint64_t m,
    const uint64_t* __restrict__ out_offsets, const uint64_t* __restrict__ totals, const uint8_t* __restrict__ comp, circkit_translate_params params,
    uint8_t* __restrict__ out)
{
    __shared__ uint8_t cls_lds[2][ck_translate::CLASS_ENTRIES];
    __shared__ uint8_t residue_lds[128];
    ck_translate::fill_tables(threadIdx.x, 64 * ck_translate::TRANSLATE_WAVES, comp, params.aa, params.unknown, cls_lds[0], cls_lds[1], residue_lds);
    __syncthreads();
    if (totals[T_REFUSED]) return;                    // the same for the whole grid
    ck_translate::Translate T;
    T.bytes = bytes; T.offsets = offsets;
    T.p0 = offsets[0]; T.p1 = offsets[n_records];
    T.windows = windows; T.out_offsets = out_offsets;
    T.m = m; T.B = totals[T_TOTAL];
    T.cls0 = cls_lds[0]; T.cls1 = cls_lds[1];
    T.residue = residue_lds;
    T.first_as_m = params.first_as_m;
    T.out = out;
    if (T.B == 0) return;
    const uint64_t n_gran = (((uint64_t)(uintptr_t)out & 15u) + T.B + 15) / 16;
    const uint64_t n_tiles = (n_gran + ck_translate::TILE_GRANULES - 1) / ck_translate::TILE_GRANULES;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) ck_translate::translate_tile(T, t);
}

__global__ __launch_bounds__(WIN_WG) void windows_of_records_kernel(const uint64_t* __restrict__ offsets, uint64_t n, uint32_t kind, int64_t bases,
                                                                    double percent, Window* __restrict__ windows)
{
    const uint64_t stride = (uint64_t)gridDim.x * WIN_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * WIN_WG + threadIdx.x; i < n; i += stride)
        windows[i] = ck_windows::window_of_record(offsets[i + 1] - offsets[i], (uint32_t)i, kind, bases, percent);
}

// ORF k lies in the record r with orf_offsets[r] <= k < orf_offsets[r + 1]; an ORF that no record's range holds (offsets that
// do not cover the list) gets a record beyond the batch: an invalid window
__global__ __launch_bounds__(WIN_WG) void orfs_windows_kernel(const uint64_t* __restrict__ orf_offsets, const circkit_orf* __restrict__ orfs,
                                                              uint64_t n_records, uint64_t n_orfs, uint32_t cut, Window* __restrict__ windows)
{
    const uint64_t stride = (uint64_t)gridDim.x * WIN_WG;
    for (uint64_t k = (uint64_t)blockIdx.x * WIN_WG + threadIdx.x; k < n_orfs; k += stride) {
        uint64_t lo = 0, hi = n_records + 1;                   // the first entry beyond k is in (lo, hi]; entry n_records + 1 = infinity
        if (orf_offsets[0] > k) hi = 0;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (orf_offsets[mid] <= k) lo = mid; else hi = mid;
        }
        const circkit_orf o = orfs[k];
        Window W;
        W.length = o.length > cut ? o.length - cut : 0;
        W.record = hi == 0 || lo >= n_records ? 0xFFFFFFFFu : (uint32_t)lo;
        W.start = o.start;
        W.strand = o.strand;
        W.reserved = 0;
        windows[k] = W;
    }
}

// the totals of the most recent gather, or of the most recent translate: each kind of call has its own
struct Totals : ck_totals {          // [T_WORDS], made at the first call of the kind
    uint64_t capacity = 0;           // of that call, for the status message
    bool any = false;
};

struct WindowsState {
    Totals gather, translate;
    ck_buf<uint64_t> d_sums;
    // the staging of circkit_windows_gather and circkit_windows_translate
    ck_csr_buf in;
    ck_buf<Window> d_win;
    ck_buf<uint64_t> d_out_off;
    ck_buf<uint8_t> d_out;
};

WindowsState* state(circkit_ctx* c) { return ck_unit_state<WindowsState>(c, CK_UNIT_WINDOWS); }

// lengths (in bytes, or in residues for a translate), the scan with its refusals, and the copy of the totals: out_offsets is
// complete and R->h valid once the stream has run past it.  d_out is only compared with the payload.
int launch_offsets(circkit_ctx* c, WindowsState* S, Totals* R, bool residues, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                   const Window* d_windows, uint64_t m, const uint8_t* d_out, uint64_t capacity, uint64_t* d_out_offsets)
{
    int rc;
    if ((rc = ck_totals_make(c, R, T_WORDS))) return rc;
    const uint64_t tiles = (m + WSCAN_TILE - 1) / WSCAN_TILE;
    if ((rc = S->d_sums.grow(c, tiles))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, R, T_WORDS))) return rc;
    if (m) {
        if (residues)
            hipLaunchKernelGGL(windows_residues_kernel, dim3(ck_grid_of(m, WIN_WG, WIN_MAX_GRID)), dim3(WIN_WG), 0, st, d_offsets, n_records, d_windows, m, d_out_offsets, R->d);
        else
            hipLaunchKernelGGL(windows_lengths_kernel, dim3(ck_grid_of(m, WIN_WG, WIN_MAX_GRID)), dim3(WIN_WG), 0, st, d_offsets, n_records, d_windows, m, d_out_offsets, R->d);
        hipLaunchKernelGGL(windows_tile_sums_kernel, dim3((uint32_t)tiles), dim3(WSCAN_WG), 0, st, (const uint64_t*)d_out_offsets + 1, m, S->d_sums);
    }
    hipLaunchKernelGGL(windows_scan_sums_kernel, dim3(1), dim3(WSCAN_WG), 0, st, S->d_sums, tiles, d_bytes, d_offsets, m ? n_records : 0, d_out, capacity,
                       d_out_offsets, R->d);
    if (m) hipLaunchKernelGGL(windows_apply_kernel, dim3((uint32_t)tiles), dim3(WSCAN_WG), 0, st, d_out_offsets + 1, m, (const uint64_t*)S->d_sums);
    CK_HIP(c, hipGetLastError());
    R->capacity = capacity;
    R->any = true;
    return CIRCKIT_OK;
}

int launch_gather(circkit_ctx* c, WindowsState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records, const Window* d_windows,
                  uint64_t m, const uint64_t* d_out_offsets, uint8_t* d_out)
{
    if (!m || !n_records) return CIRCKIT_OK;           // no window writes a byte
    hipLaunchKernelGGL(windows_gather_kernel, dim3(GATHER_GRID), dim3(64 * ck_windows::GATHER_WAVES), 0, ck_ctx_stream(c), d_bytes, d_offsets, n_records,
                       d_windows, m, d_out_offsets, (const uint64_t*)S->gather.d, ck_ctx_complement(c), d_out);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int launch_translate(circkit_ctx* c, WindowsState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records, const Window* d_windows,
                     uint64_t m, const circkit_translate_params& params, const uint64_t* d_out_offsets, uint8_t* d_out)
{
    if (!m || !n_records) return CIRCKIT_OK;           // no window writes a residue
    hipLaunchKernelGGL(windows_translate_kernel, dim3(GATHER_GRID), dim3(64 * ck_translate::TRANSLATE_WAVES), 0, ck_ctx_stream(c), d_bytes, d_offsets,
                       n_records, d_windows, m, d_out_offsets, (const uint64_t*)S->translate.d, ck_ctx_complement(c), params, d_out);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// the verdict on totals the stream has delivered
int check_totals(circkit_ctx* c, const uint64_t* t, uint64_t capacity)
{
    if (t[T_REFUSED] == REFUSED_CAPACITY)
        return ck_fail(c, CIRCKIT_ERR_OOM, "the windows write %llu bytes, the buffer holds %llu: nothing was written", (unsigned long long)t[T_TOTAL],
                       (unsigned long long)capacity);
    if (t[T_REFUSED]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_bytes overlaps the input payload: nothing was written");
    if (t[T_INVALID]) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu invalid windows were written as empty ones", (unsigned long long)t[T_INVALID]);
    return CIRCKIT_OK;
}

int check_translate_totals(circkit_ctx* c, const uint64_t* t, uint64_t capacity)
{
    if (t[T_REFUSED] == REFUSED_CAPACITY)
        return ck_fail(c, CIRCKIT_ERR_OOM, "the windows translate to %llu residues, the buffer holds %llu: nothing was written",
                       (unsigned long long)t[T_TOTAL], (unsigned long long)capacity);
    if (t[T_REFUSED]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_out_aa overlaps the input payload: nothing was written");
    if (t[T_INVALID]) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu invalid windows were translated as empty ones", (unsigned long long)t[T_INVALID]);
    return CIRCKIT_OK;
}

int check_translate_params(circkit_ctx* c, const circkit_translate_params* p)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null translate params");
    if (p->first_as_m > 1) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "first_as_m must be 0 or 1");
    for (uint8_t r : p->reserved)
        if (r) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved bytes of circkit_translate_params must be 0");
    return CIRCKIT_OK;
}

// The host form of a gather or a translate: the batch and the windows staged, the offsets first (the staging for the output is
// sized by the total they end in, so it cannot overlap the staged payload), then `launch` into that staging.  The totals
// (`kind`), `residues`, `launch` and `verdict` are the kind's own.
template <class Launch>
int host_form(circkit_ctx* c, Totals WindowsState::*kind, bool residues, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records,
              const circkit_window* windows, uint64_t n_windows, uint8_t* out, uint64_t out_capacity, uint64_t* out_offsets, uint64_t* total,
              const Launch& launch, int (*verdict)(circkit_ctx*, const uint64_t*, uint64_t))
{
    if (!out_offsets || (n_records && !offsets) || (n_windows && !windows)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records && offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    uint64_t at = 0;
    if (ck_csr_walk(offsets, n_records, CK_CSR_NO_LIMIT, &at)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (n_records && offsets[n_records] && !bytes) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_windows >= (1ull << 40) || n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_windows or n_records too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    WindowsState* S = state(c);
    Totals* R = &(S->*kind);
    int rc;
    if ((rc = S->in.upload(c, bytes, offsets, n_records))) return rc;
    if ((rc = S->d_win.upload(c, (const Window*)windows, n_windows))) return rc;
    if ((rc = S->d_out_off.grow(c, n_windows + 1))) return rc;
    if ((rc = launch_offsets(c, S, R, residues, S->in.bytes, S->in.off, n_records, S->d_win, n_windows, nullptr, out_capacity, S->d_out_off))) return rc;
    if ((rc = ck_totals_fetch(c, R, T_WORDS))) return rc;
    if ((rc = S->d_out_off.download(c, out_offsets, n_windows + 1))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    CK_HIP(c, hipStreamSynchronize(st));
    const uint64_t B = R->h[T_TOTAL];
    if (total) *total = B;
    if (R->h[T_REFUSED]) return verdict(c, R->h, out_capacity);
    if (B) {
        if (!out) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
        if ((rc = S->d_out.grow(c, B))) return rc;
        if ((rc = launch(S, S->d_out.p))) return rc;
        if ((rc = S->d_out.download(c, out, B))) return rc;
        CK_HIP(c, hipStreamSynchronize(st));
    }
    return verdict(c, R->h, out_capacity);
}

}  // namespace

extern "C" {

int circkit_windows_gather_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                  const circkit_window* d_windows, uint64_t n_windows, uint8_t* d_out_bytes, uint64_t out_capacity,
                                  uint64_t* d_out_offsets)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n_windows && (!d_windows || !d_out_offsets || (out_capacity && !d_out_bytes))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_windows && n_records && (!d_bytes || !d_offsets)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_windows >= (1ull << 40) || n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_windows or n_records too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    WindowsState* S = state(c);
    int rc;
    if ((rc = launch_offsets(c, S, &S->gather, false, d_bytes, d_offsets, n_records, (const Window*)d_windows, n_windows, d_out_bytes, out_capacity,
                             d_out_offsets)))
        return rc;
    if ((rc = launch_gather(c, S, d_bytes, d_offsets, n_records, (const Window*)d_windows, n_windows, d_out_offsets, d_out_bytes))) return rc;
    return ck_totals_fetch(c, &S->gather, T_WORDS);
}

int circkit_windows_status(circkit_ctx* c, uint64_t* total_bytes, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    WindowsState* S = state(c);
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->gather.any ? S->gather.h : none;
    if (total_bytes) *total_bytes = t[T_TOTAL];
    if (n_invalid) *n_invalid = t[T_INVALID];
    return check_totals(c, t, S->gather.capacity);
}

int circkit_windows_of_records_device(circkit_ctx* c, const uint64_t* d_offsets, uint64_t n_records, uint32_t kind, int64_t bases, double percent,
                                      circkit_window* d_windows)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (kind >= (uint32_t)ck_windows::N_KINDS) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "unknown kind of window");
    if ((kind == CIRCKIT_WINDOWS_ROTATE_BASES && bases == 0) || (kind == CIRCKIT_WINDOWS_ROTATE_PERCENT && percent == 0.0))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "Rotation by 0 is not allowed");       // src/rotate.rs:20-22
    if (n_records && (!d_offsets || !d_windows)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records > 0xFFFFFFFFull) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "a window names its record in 32 bits: n_records must be <= 2^32 - 1");
    if (!n_records) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    hipLaunchKernelGGL(windows_of_records_kernel, dim3(ck_grid_of(n_records, WIN_WG, WIN_MAX_GRID)), dim3(WIN_WG), 0, ck_ctx_stream(c), d_offsets, n_records, kind, bases, percent,
                       (Window*)d_windows);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int circkit_orfs_windows_device(circkit_ctx* c, const uint64_t* d_orf_offsets, const circkit_orf* d_orfs, uint64_t n_records, uint64_t n_orfs,
                                int include_stop, circkit_window* d_windows)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (n_orfs && (!d_orf_offsets || !d_orfs || !d_windows)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records > 0xFFFFFFFFull) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "a window names its record in 32 bits: n_records must be <= 2^32 - 1");
    if (n_orfs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_orfs too large");
    if (!n_orfs) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    hipLaunchKernelGGL(orfs_windows_kernel, dim3(ck_grid_of(n_orfs, WIN_WG, WIN_MAX_GRID)), dim3(WIN_WG), 0, ck_ctx_stream(c), d_orf_offsets, d_orfs, n_records, n_orfs,
                       include_stop ? 0u : 3u, (Window*)d_windows);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int circkit_windows_gather(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, const circkit_window* windows,
                           uint64_t n_windows, uint8_t* out_bytes, uint64_t out_capacity, uint64_t* out_offsets, uint64_t* total)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    return host_form(c, &WindowsState::gather, false, bytes, offsets, n_records, windows, n_windows, out_bytes, out_capacity, out_offsets, total,
                     [&](WindowsState* S, uint8_t* d_out) { return launch_gather(c, S, S->in.bytes, S->in.off, n_records, S->d_win, n_windows, S->d_out_off, d_out); },
                     check_totals);
}

int circkit_windows_translate_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n_records,
                                     const circkit_window* d_windows, uint64_t n_windows, const circkit_translate_params* params, uint8_t* d_out_aa,
                                     uint64_t out_capacity, uint64_t* d_out_offsets)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_translate_params(c, params))) return rc;
    if (n_windows && (!d_windows || !d_out_offsets || (out_capacity && !d_out_aa))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_windows && n_records && (!d_bytes || !d_offsets)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_windows >= (1ull << 40) || n_records >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_windows or n_records too large");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    WindowsState* S = state(c);
    if ((rc = launch_offsets(c, S, &S->translate, true, d_bytes, d_offsets, n_records, (const Window*)d_windows, n_windows, d_out_aa, out_capacity,
                             d_out_offsets)))
        return rc;
    if ((rc = launch_translate(c, S, d_bytes, d_offsets, n_records, (const Window*)d_windows, n_windows, *params, d_out_offsets, d_out_aa))) return rc;
    return ck_totals_fetch(c, &S->translate, T_WORDS);
}

int circkit_translate_status(circkit_ctx* c, uint64_t* total_residues, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    WindowsState* S = state(c);
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[T_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->translate.any ? S->translate.h : none;
    if (total_residues) *total_residues = t[T_TOTAL];
    if (n_invalid) *n_invalid = t[T_INVALID];
    return check_translate_totals(c, t, S->translate.capacity);
}

int circkit_windows_translate(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, const circkit_window* windows,
                              uint64_t n_windows, const circkit_translate_params* params, uint8_t* out_aa, uint64_t out_capacity,
                              uint64_t* out_offsets, uint64_t* total)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_translate_params(c, params))) return rc;
    return host_form(c, &WindowsState::translate, true, bytes, offsets, n_records, windows, n_windows, out_aa, out_capacity, out_offsets, total,
                     [&](WindowsState* S, uint8_t* d_out) {
                         return launch_translate(c, S, S->in.bytes, S->in.off, n_records, S->d_win, n_windows, *params, S->d_out_off, d_out);
                     },
                     check_translate_totals);
}

}  // extern "C"
