// circkit_cluster.hip -- candidate pairs from sketch rows and single linkage over scored pairs: the "clusters of circular records"
// section of include/circkit.h.  The routines are cluster.h's; here are the kernels around them, the unit's state and the ABI.
//
// Candidates are seven launches on the ctx stream and the uniq unit's resolve between the first and the second; nothing waits:
//   cluster_keys_kernel       one lane per (record, band), striding: the band keys
//   circkit_uniq_resolve_device over the keys: the smallest position with an equal key (the ctx's uniq table, through the C ABI)
//   cluster_count_kernel      one wave per record, striding: the mask of the proposing bands and their number
//   cluster_tile_sums_kernel / cluster_scan_sums_kernel / cluster_apply_kernel   ck_scan.h's three bodies with the saturating
//                             sum: the numbers become d_pair_offsets in place; the middle one keeps the total
//   cluster_write_kernel      one wave per record, striding: the pairs of every record that fits below the capacity
// A link is three: cluster_init_kernel (parent[i] = i), cluster_link_kernel (one lane per pair, striding: threshold and union),
// cluster_flatten_kernel (labels and the number of roots).  No kernel uses LDS beyond the scan's and no workgroup waits for another.
// The totals of either kind are the unit's own: they stay in device memory and are copied to page-locked memory behind the
// work, and circkit_cluster_candidates_status / circkit_cluster_link_status answer from them whatever other unit ran in between:
// the overflow count of the candidates' resolve is copied into their totals behind the resolve, one 4-byte copy on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "ck_csr.h"
#include "ck_ctx.h"
#include "ck_scan.h"
#include "cluster.h"

using ck_cluster::Emit;
using ck_cluster::Keys;
using ck_cluster::Link;
using ck_cluster::C_WORDS;
using ck_cluster::L_WORDS;

static_assert(sizeof(circkit_cluster_params) == 24, "params layout");

namespace {

constexpr int KEYS_WG = 256;
constexpr uint32_t KEYS_MAX_GRID = 4096;               // workgroups of the keys kernel: the lanes stride over the (record, band) positions
constexpr uint32_t EMIT_WAVES = 4, EMIT_MAX_GRID = 4096;   // of the count and write kernels: the waves stride over the records
constexpr int SCAN_WG = (int)ck_cluster::SCAN_WG, SCAN_ITEMS = (int)ck_cluster::SCAN_ITEMS, SCAN_TILE = (int)ck_cluster::SCAN_TILE;
constexpr int LINK_WG = 256;
constexpr uint32_t LINK_MAX_GRID = 2048;               // of the link kernel: the lanes stride over the pairs
constexpr uint32_t FLATTEN_MAX_GRID = 2048;            // of the init and flatten kernels (LINK_WG lanes): the lanes stride over the records

__global__ __launch_bounds__(KEYS_WG) void cluster_keys_kernel(Keys K)
{
    ck_cluster::keys_lane(K, (uint64_t)blockIdx.x * KEYS_WG + threadIdx.x, (uint64_t)gridDim.x * KEYS_WG);
}

__global__ __launch_bounds__(64 * EMIT_WAVES) void cluster_count_kernel(Emit E)
{
    ck_cluster::count_wave(E, (uint64_t)blockIdx.x * EMIT_WAVES + ck::wave_in_block(), (uint64_t)gridDim.x * EMIT_WAVES);
}

__global__ __launch_bounds__(SCAN_WG) void cluster_tile_sums_kernel(const uint64_t* __restrict__ len, uint64_t n, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    const uint64_t total = ck_scan::tile_sum<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, len, n, [](uint64_t w) { return w; }, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: the tile sums become exclusive, SCAN_WG of them a round; then the total and d_pair_offsets[0].
__global__ __launch_bounds__(SCAN_WG) void cluster_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t n_tiles, uint64_t* __restrict__ offsets,
                                                                    uint64_t* __restrict__ totals)
{
    __shared__ uint64_t lds[SCAN_WG];
    const uint64_t total = ck_scan::sums_exclusive<SCAN_WG, ck_scan::SatAdd>(threadIdx.x, sums, n_tiles, lds);
    if (threadIdx.x == 0) {
        totals[ck_cluster::C_TOTAL] = total;
        offsets[0] = 0;
    }
}

__global__ __launch_bounds__(SCAN_WG) void cluster_apply_kernel(uint64_t* __restrict__ ends, uint64_t n, const uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    ck_scan::apply_ends<SCAN_WG, SCAN_ITEMS, ck_scan::SatAdd>(threadIdx.x, blockIdx.x, ends, n, sums, lds);
}

__global__ __launch_bounds__(64 * EMIT_WAVES) void cluster_write_kernel(Emit E)
{
    ck_cluster::write_wave(E, (uint64_t)blockIdx.x * EMIT_WAVES + ck::wave_in_block(), (uint64_t)gridDim.x * EMIT_WAVES);
}

__global__ __launch_bounds__(LINK_WG) void cluster_init_kernel(Link L)
{
    ck_cluster::init_lane(L, (uint64_t)blockIdx.x * LINK_WG + threadIdx.x, (uint64_t)gridDim.x * LINK_WG);
}

__global__ __launch_bounds__(LINK_WG) void cluster_link_kernel(Link L)
{
    ck_cluster::link_lane(L, (uint64_t)blockIdx.x * LINK_WG + threadIdx.x, (uint64_t)gridDim.x * LINK_WG);
}

__global__ __launch_bounds__(LINK_WG) void cluster_flatten_kernel(Link L)
{
    ck_cluster::flatten_lane(L, (uint64_t)blockIdx.x * LINK_WG + threadIdx.x, (uint64_t)gridDim.x * LINK_WG);
}

struct ClusterState {
    ck_totals cand;                  // [C_WORDS], of the most recent candidates call; both made with the state
    ck_totals link;                  // [L_WORDS], of the most recent link
    bool any_cand = false, any_link = false;
    uint64_t capacity = 0;           // of the most recent candidates call
    ck_buf<uint64_t> d_keys, d_first;        // n_records * n_bands
    ck_buf<uint64_t> d_masks, d_sums;
    ck_buf<uint32_t> d_parent;
    // the staging of circkit_cluster_batch
    ck_csr_buf in;
    ck_buf<uint64_t> d_rows, d_pair_off, d_labels;
    ck_buf<uint32_t> d_pairs, d_scores;
};

int state(circkit_ctx* c, ClusterState** out)
{
    ClusterState* S = *out = ck_unit_state<ClusterState>(c, CK_UNIT_CLUSTER);
    int rc;
    if ((rc = ck_totals_make(c, &S->cand, C_WORDS))) return rc;
    return ck_totals_make(c, &S->link, L_WORDS);
}

int check_params(circkit_ctx* c, const circkit_cluster_params* p)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null cluster params");
    if (p->n_bands < 1 || p->n_bands > ck_cluster::N_BANDS_MAX) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_bands must be 1 .. 64");
    if (p->band_bins < 1 || p->band_bins > ck_cluster::BAND_BINS_MAX) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "band_bins must be 1 .. 16");
    if (p->min_similarity_q16 > 65536) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "min_similarity_q16 must be 0 .. 65536");
    if (p->min_filled < 1) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "min_filled must be at least 1");
    if (p->reserved[0] || p->reserved[1]) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "the reserved words of circkit_cluster_params must be 0");
    return CIRCKIT_OK;
}

// what the candidates ask beyond check_params
int check_bands(circkit_ctx* c, const circkit_cluster_params* p, uint32_t log2_bins, uint64_t n)
{
    if (log2_bins < ck_sketch::LOG2_BINS_MIN || log2_bins > ck_sketch::LOG2_BINS_MAX)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "log2_bins must be 4 .. 10");
    if (p->n_bands * p->band_bins > (1u << log2_bins)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_bands * band_bins exceeds the bins of a row");
    if (n >= (1ull << 32) || n * p->n_bands >= 0xFFFFFFFFull)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records * n_bands must be < 2^32 - 1");
    return CIRCKIT_OK;
}

// the launches of the candidates and the copy of the total; the arguments are checked
int launch_candidates(circkit_ctx* c, ClusterState* S, const uint64_t* d_sketch, uint64_t n, uint32_t log2_bins, const circkit_cluster_params& p,
                      uint64_t* d_pair_offsets, uint32_t* d_pairs, uint64_t capacity)
{
    const uint64_t n_keys = n * p.n_bands, tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    int rc;
    if ((rc = S->d_keys.grow(c, n_keys))) return rc;
    if ((rc = S->d_first.grow(c, n_keys))) return rc;
    if ((rc = S->d_masks.grow(c, n))) return rc;
    if ((rc = S->d_sums.grow(c, tiles))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, &S->cand, C_WORDS))) return rc;
    Emit E;
    E.keys = S->d_keys; E.first_pos = S->d_first; E.n_records = n; E.n_bands = p.n_bands;
    E.masks = S->d_masks; E.offsets = d_pair_offsets; E.pairs = d_pairs; E.capacity = capacity;
    if (n) {
        Keys K;
        K.rows = d_sketch; K.n_records = n; K.log2_bins = log2_bins; K.n_bands = p.n_bands; K.band_bins = p.band_bins; K.keys = S->d_keys;
        hipLaunchKernelGGL(cluster_keys_kernel, dim3(ck_grid_of(n_keys, KEYS_WG, KEYS_MAX_GRID)), dim3(KEYS_WG), 0, st, K);
        CK_HIP(c, hipGetLastError());
        if ((rc = circkit_uniq_resolve_device(c, S->d_keys, n_keys, 0, S->d_first, nullptr))) return rc;
        // the resolve's overflow count while it is still this call's: the table is anybody's after the next circkit_uniq_reset
        const uint32_t* d_overflow;
        if ((rc = ck_uniq_overflow_word(c, &d_overflow))) return rc;
        CK_HIP(c, hipMemcpyAsync(S->cand.d + ck_cluster::C_OVERFLOW, d_overflow, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(cluster_count_kernel, dim3(ck_grid_of(n, EMIT_WAVES, EMIT_MAX_GRID)), dim3(64 * EMIT_WAVES), 0, st, E);
        hipLaunchKernelGGL(cluster_tile_sums_kernel, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, (const uint64_t*)d_pair_offsets + 1, n, S->d_sums);
    }
    hipLaunchKernelGGL(cluster_scan_sums_kernel, dim3(1), dim3(SCAN_WG), 0, st, S->d_sums, tiles, d_pair_offsets, S->cand.d);
    if (n) {
        hipLaunchKernelGGL(cluster_apply_kernel, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, d_pair_offsets + 1, n, (const uint64_t*)S->d_sums);
        hipLaunchKernelGGL(cluster_write_kernel, dim3(ck_grid_of(n, EMIT_WAVES, EMIT_MAX_GRID)), dim3(64 * EMIT_WAVES), 0, st, E);
    }
    CK_HIP(c, hipGetLastError());
    if ((rc = ck_totals_fetch(c, &S->cand, C_WORDS))) return rc;
    S->capacity = capacity;
    S->any_cand = true;
    return CIRCKIT_OK;
}

int check_candidates(circkit_ctx* c, uint64_t total, uint64_t capacity)
{
    if (total > capacity)
        return ck_fail(c, CIRCKIT_ERR_OOM, "%llu candidate pairs do not fit the capacity of %llu: the records beyond it were not written",
                       (unsigned long long)total, (unsigned long long)capacity);
    return CIRCKIT_OK;
}

int launch_link(circkit_ctx* c, ClusterState* S, uint64_t n, const uint32_t* d_pairs, const uint32_t* d_scores, uint64_t n_pairs,
                const circkit_cluster_params& p, uint64_t* d_labels)
{
    int rc;
    if ((rc = S->d_parent.grow(c, n))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = ck_totals_clear(c, &S->link, L_WORDS))) return rc;
    Link L;
    L.n_records = n; L.pairs = d_pairs; L.scores = d_scores; L.n_pairs = n_pairs;
    L.min_similarity_q16 = p.min_similarity_q16; L.min_filled = p.min_filled;
    L.parent = S->d_parent; L.labels = d_labels; L.totals = S->link.d;
    if (n) hipLaunchKernelGGL(cluster_init_kernel, dim3(ck_grid_of(n, LINK_WG, FLATTEN_MAX_GRID)), dim3(LINK_WG), 0, st, L);
    if (n_pairs) hipLaunchKernelGGL(cluster_link_kernel, dim3(ck_grid_of(n_pairs, LINK_WG, LINK_MAX_GRID)), dim3(LINK_WG), 0, st, L);
    if (n) hipLaunchKernelGGL(cluster_flatten_kernel, dim3(ck_grid_of(n, LINK_WG, FLATTEN_MAX_GRID)), dim3(LINK_WG), 0, st, L);
    CK_HIP(c, hipGetLastError());
    if ((rc = ck_totals_fetch(c, &S->link, L_WORDS))) return rc;
    S->any_link = true;
    return CIRCKIT_OK;
}

int check_link(circkit_ctx* c, const uint64_t* t)
{
    if (t[ck_cluster::L_INVALID])
        return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "%llu pairs name a record that does not exist and were skipped", (unsigned long long)t[ck_cluster::L_INVALID]);
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_cluster_candidates_device(circkit_ctx* c, const uint64_t* d_sketch, uint64_t n_records, uint32_t log2_bins,
                                      const circkit_cluster_params* params, uint64_t* d_pair_offsets, uint32_t* d_pairs, uint64_t capacity)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if ((rc = check_bands(c, params, log2_bins, n_records))) return rc;
    if (!d_pair_offsets || (n_records && !d_sketch) || (capacity && !d_pairs)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_sketch & 7u) || ((uintptr_t)d_pair_offsets & 7u) || ((uintptr_t)d_pairs & 3u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_sketch and d_pair_offsets must be 8-byte aligned, d_pairs 4-byte aligned");
    if (capacity >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "capacity too large");
    const uint64_t row_bytes = (n_records << log2_bins) * sizeof(uint64_t), off_bytes = (n_records + 1) * sizeof(uint64_t),
                   pair_bytes = capacity * 2 * sizeof(uint32_t);
    if (ck_overlap(d_pair_offsets, off_bytes, d_sketch, row_bytes) || ck_overlap(d_pairs, pair_bytes, d_sketch, row_bytes) ||
        ck_overlap(d_pairs, pair_bytes, d_pair_offsets, off_bytes))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_pair_offsets / d_pairs overlap the sketch or each other");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    ClusterState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_candidates(c, S, d_sketch, n_records, log2_bins, *params, d_pair_offsets, d_pairs, capacity);
}

int circkit_cluster_candidates_status(circkit_ctx* c, uint64_t* total_pairs)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    ClusterState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t total = S->any_cand ? S->cand.h[ck_cluster::C_TOTAL] : 0;
    if (total_pairs) *total_pairs = total;
    const uint32_t overflow = S->any_cand ? (uint32_t)S->cand.h[ck_cluster::C_OVERFLOW] : 0;      // of this call's own resolve
    if (overflow)                                                                                // keys that found no slot proposed nothing
        return ck_fail(c, CIRCKIT_ERR_OOM, "uniq table overflow: %u key(s) found no slot (more distinct keys than circkit_uniq_reset sized it for)", overflow);
    return check_candidates(c, total, S->any_cand ? S->capacity : 0);
}

int circkit_cluster_link_device(circkit_ctx* c, uint64_t n_records, const uint32_t* d_pairs, const uint32_t* d_scores, uint64_t n_pairs,
                                const circkit_cluster_params* params, uint64_t* d_labels)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (n_records >= (1ull << 32)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records must be < 2^32");
    if (n_pairs >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_pairs too large");
    if ((n_records && !d_labels) || (n_pairs && (!d_pairs || !d_scores))) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (((uintptr_t)d_pairs & 3u) || ((uintptr_t)d_scores & 3u) || ((uintptr_t)d_labels & 7u))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_pairs and d_scores must be 4-byte aligned, d_labels 8-byte aligned");
    const uint64_t pair_bytes = n_pairs * 2 * sizeof(uint32_t), label_bytes = n_records * sizeof(uint64_t);
    if (ck_overlap(d_labels, label_bytes, d_pairs, pair_bytes) || ck_overlap(d_labels, label_bytes, d_scores, pair_bytes))
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "d_labels overlaps the pairs or the scores");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    ClusterState* S;
    if ((rc = state(c, &S))) return rc;
    return launch_link(c, S, n_records, d_pairs, d_scores, n_pairs, *params, d_labels);
}

int circkit_cluster_link_status(circkit_ctx* c, uint64_t* n_clusters, uint64_t* n_linked, uint64_t* n_invalid)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    ClusterState* S;
    int rc;
    if ((rc = state(c, &S))) return rc;
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t none[L_WORDS] = { 0, 0, 0 };
    const uint64_t* t = S->any_link ? S->link.h : none;
    if (n_clusters) *n_clusters = t[ck_cluster::L_CLUSTERS];
    if (n_linked) *n_linked = t[ck_cluster::L_LINKED];
    if (n_invalid) *n_invalid = t[ck_cluster::L_INVALID];
    return check_link(c, t);
}

int circkit_cluster_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, const circkit_sketch_params* sketch,
                          const circkit_cluster_params* params, uint64_t* labels, uint64_t* n_clusters)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    int rc;
    if ((rc = check_params(c, params))) return rc;
    if (!sketch) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null sketch params");
    if (sketch->k < ck_sketch::K_MIN || sketch->k > ck_sketch::K_MAX || sketch->reserved[0] || sketch->reserved[1])
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "k must be 4 .. 32 and the reserved words of circkit_sketch_params 0");
    if ((rc = check_bands(c, params, sketch->log2_bins, n_records))) return rc;
    if (n_records && (!offsets || !labels)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n_records && offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    // from the offsets alone, before a payload byte is read
    uint64_t at = 0;
    const ck_csr_fault fault = ck_csr_walk(offsets, n_records, ck_sketch::TOO_LONG, &at);
    if (fault == CK_CSR_DECREASE) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets must not decrease");
    if (fault) return ck_fail(c, CIRCKIT_ERR_TOO_LONG, "record %llu has 2^31 symbols or more: nothing was clustered", (unsigned long long)at);
    const uint64_t nb = n_records ? offsets[n_records] : 0;
    if (nb && !bytes) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    ClusterState* S;
    if ((rc = state(c, &S))) return rc;
    if (n_clusters) *n_clusters = 0;
    const uint64_t n_rows = n_records << sketch->log2_bins, capacity = n_records * params->n_bands;
    if ((rc = S->in.upload(c, bytes, offsets, n_records))) return rc;
    if ((rc = S->d_rows.grow(c, n_rows))) return rc;
    if ((rc = S->d_pair_off.grow(c, n_records + 1))) return rc;
    if ((rc = S->d_pairs.grow(c, 2 * capacity))) return rc;
    if ((rc = S->d_scores.grow(c, 2 * capacity))) return rc;
    if ((rc = S->d_labels.grow(c, n_records))) return rc;
    if ((rc = circkit_sketch_batch_device(c, S->in.bytes, S->in.off, n_records, sketch, S->d_rows, nullptr))) return rc;
    if ((rc = launch_candidates(c, S, S->d_rows, n_records, sketch->log2_bins, *params, S->d_pair_off, S->d_pairs, capacity))) return rc;
    // the one wait in the middle: the compare takes the number of pairs from the host
    uint64_t n_pairs = 0;
    if ((rc = circkit_cluster_candidates_status(c, &n_pairs))) return rc;
    if ((rc = circkit_sketch_compare_device(c, S->d_rows, n_records, S->d_rows, n_records, sketch->log2_bins, S->d_pairs, n_pairs, S->d_scores))) return rc;
    if ((rc = launch_link(c, S, n_records, S->d_pairs, S->d_scores, n_pairs, *params, S->d_labels))) return rc;
    if ((rc = S->d_labels.download(c, labels, n_records))) return rc;
    if ((rc = circkit_sketch_status(c, nullptr, nullptr))) return rc;
    if ((rc = circkit_sketch_compare_status(c, nullptr))) return rc;
    if ((rc = check_link(c, S->link.h))) return rc;
    if (n_clusters) *n_clusters = S->link.h[ck_cluster::L_CLUSTERS];
    return CIRCKIT_OK;
}

}  // extern "C"
