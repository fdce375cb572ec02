// circkit_orfs.hip -- `circkit orfs` on the GPU: the batch entry points of include/circkit.h's ORF section.
//
// A batch is three steps on the ctx stream, so that every record's ORFs land at offsets in record order:
//   orfs_count_kernel   one lane per record runs orf_strand (orfs.h) on each requested strand and writes the count
//   scan                exclusive prefix sum of the counts into d_orf_offsets (tile sums, one-workgroup scan, apply)
//   orfs_emit_kernel    the same lane runs the same sweep again, writes the descriptors at its offset and sorts each
//                       strand's run into the reference's output order (orfs.h sort_run: insertion sort up to 32,
//                       heapsort beyond)
// A lane per record reads its record twice per strand (prologue + sweep) in each of the two passes; the bytes are L2-resident
// between passes for the records of a workgroup.  Records of fewer than 2 symbols have no ORFs (the reference panics on
// them; the CLI reports that itself), records of 2^32 symbols or more are not processed (none are produced).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/circkit.h"
#include "ck_ctx.h"            // the ctx lives in circkit_hip.hip; this file sees it through this header
#include "ck_scan.h"
#include "orfs.h"

using ck_orfs::Orf;
using ck_orfs::Filter;

static_assert(sizeof(Orf) == sizeof(circkit_orf), "device ORF layout");


namespace {

constexpr int ORF_WG = 256;
constexpr int SCAN_WG = 1024, SCAN_ITEMS = 8, SCAN_TILE = SCAN_WG * SCAN_ITEMS;      // the scan of the counts (ck_scan.h)

struct OrfArgs {
    uint8_t cls[512];        // codon class table: bit 0 start set, bit 1 stop set
    Filter F;
    uint32_t strands;        // bit 0 forward, bit 1 reverse
};

__device__ inline uint32_t record_orfs(const uint8_t* __restrict__ s, uint64_t L, const uint8_t* cls, const OrfArgs& A,
                                       Orf* out, uint32_t* n_fwd)
{
    uint32_t n = 0;
    *n_fwd = 0;
    if (L < 2 || L > 0xFFFFFFFFull) return 0;
    const uint32_t L32 = (uint32_t)L;
    auto put = [&](const Orf& o) { if (out) out[n] = o; ++n; };
    if (A.strands & 1) {
        ck_orfs::orf_strand<false>(s, L32, cls, A.F, 0, put);
        *n_fwd = n;
    }
    if (A.strands & 2) ck_orfs::orf_strand<true>(s, L32, cls, A.F, 1, put);
    return n;
}

__global__ __launch_bounds__(ORF_WG) void orfs_count_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                            uint64_t n, OrfArgs A, uint64_t* __restrict__ orf_offsets)
{
    __shared__ uint8_t cls[512];
    for (int k = threadIdx.x; k < 512; k += blockDim.x) cls[k] = A.cls[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * ORF_WG + threadIdx.x;
    if (i == 0) orf_offsets[0] = 0;
    if (i >= n) return;
    const uint64_t o = offsets[i], L = offsets[i + 1] - o;
    uint32_t nf;
    orf_offsets[i + 1] = record_orfs(bytes + o, L, cls, A, nullptr, &nf);
}

__global__ __launch_bounds__(ORF_WG) void orfs_emit_kernel(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                           uint64_t n, OrfArgs A, const uint64_t* __restrict__ orf_offsets,
                                                           Orf* __restrict__ orfs, uint64_t capacity)
{
    __shared__ uint8_t cls[512];
    for (int k = threadIdx.x; k < 512; k += blockDim.x) cls[k] = A.cls[k];
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * ORF_WG + threadIdx.x;
    if (i >= n) return;
    const uint64_t base = orf_offsets[i], end = orf_offsets[i + 1];
    // a record whose ORFs do not all fit is not written; end < base (offsets that a failed scan left falling) is not
    // either, where (end - base) - nf below would wrap and the sort would run far past the buffer
    if (end <= base || end > capacity) return;
    const uint64_t o = offsets[i], L = offsets[i + 1] - o;
    uint32_t nf;
    record_orfs(bytes + o, L, cls, A, orfs + base, &nf);
    ck_orfs::sort_run(orfs + base, nf, A.F.mode);
    ck_orfs::sort_run(orfs + base + nf, (uint32_t)(end - base) - nf, A.F.mode);
}

// ---- exclusive scan of uint64 counts, in place: a[0..n) (a[-1] is the 0 the count kernel wrote); the bodies are ck_scan.h's ----
__global__ __launch_bounds__(SCAN_WG) void scan_tile_sums(const uint64_t* __restrict__ a, uint64_t n, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    const uint64_t total = ck_scan::tile_sum<SCAN_WG, SCAN_ITEMS, ck_scan::Add>(threadIdx.x, blockIdx.x, a, n, [](uint64_t w) { return w; }, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_WG) void scan_sums(uint64_t* __restrict__ sums, uint64_t n_tiles)
{
    __shared__ uint64_t lds[SCAN_WG];
    ck_scan::sums_exclusive<SCAN_WG, ck_scan::Add>(threadIdx.x, sums, n_tiles, lds);
}

// inclusive over counts = exclusive over records (a = offsets + 1)
__global__ __launch_bounds__(SCAN_WG) void scan_apply(uint64_t* __restrict__ a, uint64_t n, const uint64_t* __restrict__ sums)
{
    __shared__ uint64_t lds[SCAN_WG];
    ck_scan::apply_ends<SCAN_WG, SCAN_ITEMS, ck_scan::Add>(threadIdx.x, blockIdx.x, a, n, sums, lds);
}

struct OrfState {
    uint64_t* h_total = nullptr;      // pinned: d_orf_offsets[n] of the last device batch
    uint64_t capacity = 0;
    bool host_last = false;           // the last batch was the host form: its total is host_total
    uint64_t host_total = 0;
    ck_buf<uint64_t> d_sums;
    // host-buffer form staging
    ck_csr_buf in;
    ck_buf<uint64_t> d_orf_off;
    ck_buf<Orf> d_orfs;
    ~OrfState() { if (h_total) (void)hipHostFree(h_total); }
};

OrfState* state(circkit_ctx* c) { return ck_unit_state<OrfState>(c, CK_UNIT_ORFS); }

int make_args(circkit_ctx* c, const circkit_orf_params* p, OrfArgs* A)
{
    if (!p) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null params");
    if (p->n_start_codons > CIRCKIT_ORF_MAX_CODONS || p->n_stop_codons > CIRCKIT_ORF_MAX_CODONS)
        return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "more than 64 start or stop codons");
    if (p->mode > 1 || (p->strands & ~3u)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "bad mode or strand mask");
    memset(A, 0, sizeof *A);
    auto add = [&](const uint8_t (*codons)[3], uint32_t n, uint8_t bit) {
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t a = ck_orfs::sym_code(codons[k][0]), b = ck_orfs::sym_code(codons[k][1]), d = ck_orfs::sym_code(codons[k][2]);
            if (a == 6 || b == 6 || d == 6) continue;            // a byte no normalized record holds: never matches
            A->cls[(a << 6) | (b << 3) | d] |= bit;
        }
    };
    add(p->start_codons, p->n_start_codons, ck_orfs::CLS_START);
    add(p->stop_codons, p->n_stop_codons, ck_orfs::CLS_STOP);
    A->F.min_length = p->min_length;
    A->F.min_ratio = p->min_ratio;
    A->F.min_wraps = p->min_wraps;
    A->F.max_wraps = p->max_wraps;
    A->F.require_stop = p->require_stop ? 1 : 0;
    A->F.mode = p->mode;
    A->strands = p->strands;
    return CIRCKIT_OK;
}

// count + scan; the offsets are complete once the stream has run past it
int launch_count(circkit_ctx* c, OrfState* S, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const OrfArgs& A,
                 uint64_t* d_orf_offsets)
{
    hipStream_t st = ck_ctx_stream(c);
    const uint64_t grid = n ? (n + ORF_WG - 1) / ORF_WG : 1;
    hipLaunchKernelGGL(orfs_count_kernel, dim3((uint32_t)grid), dim3(ORF_WG), 0, st, d_bytes, d_offsets, n, A, d_orf_offsets);
    CK_HIP(c, hipGetLastError());
    if (n == 0) return CIRCKIT_OK;
    const uint64_t tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
    int rc = S->d_sums.grow(c, tiles);
    if (rc) return rc;
    hipLaunchKernelGGL(scan_tile_sums, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, (const uint64_t*)d_orf_offsets + 1, n, S->d_sums);
    hipLaunchKernelGGL(scan_sums, dim3(1), dim3(SCAN_WG), 0, st, S->d_sums, tiles);
    hipLaunchKernelGGL(scan_apply, dim3((uint32_t)tiles), dim3(SCAN_WG), 0, st, d_orf_offsets + 1, n, (const uint64_t*)S->d_sums);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int launch_emit(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const OrfArgs& A,
                const uint64_t* d_orf_offsets, Orf* d_orfs, uint64_t capacity)
{
    if (n == 0 || !d_orfs || capacity == 0) return CIRCKIT_OK;
    const uint64_t grid = (n + ORF_WG - 1) / ORF_WG;
    hipLaunchKernelGGL(orfs_emit_kernel, dim3((uint32_t)grid), dim3(ORF_WG), 0, ck_ctx_stream(c), d_bytes, d_offsets, n, A,
                       d_orf_offsets, d_orfs, capacity);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

}  // namespace

extern "C" {

int circkit_orfs_batch_device(circkit_ctx* c, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                              const circkit_orf_params* params, uint64_t* d_orf_offsets, circkit_orf* d_orfs, uint64_t capacity)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!d_offsets || !d_orf_offsets || (n && !d_bytes)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (n >= (1ull << 40)) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "n_records too large");
    OrfArgs A;
    int rc = make_args(c, params, &A);
    if (rc) return rc;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    OrfState* S = state(c);
    if (!S->h_total) CK_HIP(c, hipHostMalloc((void**)&S->h_total, sizeof(uint64_t), hipHostMallocDefault));
    rc = launch_count(c, S, d_bytes, d_offsets, n, A, d_orf_offsets);
    if (rc) return rc;
    rc = launch_emit(c, d_bytes, d_offsets, n, A, d_orf_offsets, (Orf*)d_orfs, capacity);
    if (rc) return rc;
    CK_HIP(c, hipMemcpyAsync(S->h_total, d_orf_offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, ck_ctx_stream(c)));
    S->capacity = capacity;
    S->host_last = false;
    return CIRCKIT_OK;
}

int circkit_orfs_status(circkit_ctx* c, uint64_t* total)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    OrfState* S = state(c);
    CK_HIP(c, hipStreamSynchronize(ck_ctx_stream(c)));
    const uint64_t t = S->host_last ? S->host_total : S->h_total ? *S->h_total : 0;
    if (total) *total = t;
    if (t > S->capacity) {
        char m[160];
        snprintf(m, sizeof m, "the batch has %llu ORFs, the buffer holds %llu", (unsigned long long)t, (unsigned long long)S->capacity);
        return ck_ctx_fail(c, CIRCKIT_ERR_OOM, m);
    }
    return CIRCKIT_OK;
}

int circkit_orfs_batch(circkit_ctx* c, const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const circkit_orf_params* params,
                       uint64_t* orf_offsets, circkit_orf* orfs, uint64_t capacity, uint64_t* total)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!offsets || !orf_offsets || (n && !bytes && offsets[n] > offsets[0])) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null buffer");
    if (offsets[0] != 0) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "offsets[0] must be 0");
    OrfArgs A;
    int rc = make_args(c, params, &A);
    if (rc) return rc;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    OrfState* S = state(c);
    if ((rc = S->in.upload(c, bytes, offsets, n))) return rc;        // (of an empty batch no offset is read)
    if ((rc = S->d_orf_off.grow(c, n + 1))) return rc;
    hipStream_t st = ck_ctx_stream(c);
    if ((rc = launch_count(c, S, S->in.bytes, S->in.off, n, A, S->d_orf_off))) return rc;
    if ((rc = S->d_orf_off.download(c, orf_offsets, n + 1))) return rc;
    CK_HIP(c, hipStreamSynchronize(st));
    const uint64_t t = orf_offsets[n];
    if (total) *total = t;
    S->host_last = true; S->host_total = t; S->capacity = capacity;
    if (t > capacity) {
        char m[160];
        snprintf(m, sizeof m, "the batch has %llu ORFs, the buffer holds %llu", (unsigned long long)t, (unsigned long long)capacity);
        return ck_ctx_fail(c, CIRCKIT_ERR_OOM, m);
    }
    if (t == 0) return CIRCKIT_OK;
    if ((rc = S->d_orfs.grow(c, t))) return rc;
    if ((rc = launch_emit(c, S->in.bytes, S->in.off, n, A, S->d_orf_off, S->d_orfs, t))) return rc;
    CK_HIP(c, hipMemcpyAsync(orfs, S->d_orfs, t * sizeof(Orf), hipMemcpyDeviceToHost, st));      // (a null orfs is HIP's to refuse)
    CK_HIP(c, hipStreamSynchronize(st));
    return CIRCKIT_OK;
}

int circkit_find_orfs(circkit_ctx* c, const uint8_t* s, size_t n, circkit_orf* out, size_t capacity, size_t* count)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    if (!s && n) return ck_ctx_fail(c, CIRCKIT_ERR_INVALID_ARG, "null sequence");
    circkit_orf_params p;
    memset(&p, 0, sizeof p);
    memcpy(p.start_codons[0], "ATG", 3);
    p.n_start_codons = 1;
    memcpy(p.stop_codons[0], "TAA", 3); memcpy(p.stop_codons[1], "TAG", 3); memcpy(p.stop_codons[2], "TGA", 3);
    p.n_stop_codons = 3;
    p.min_length = 0; p.min_ratio = 0.0; p.min_wraps = 0; p.max_wraps = 3; p.require_stop = 0;
    p.strands = 1; p.mode = 1;
    const uint64_t offs[2] = { 0, (uint64_t)n };
    uint64_t orf_offs[2] = { 0, 0 }, total = 0;
    const int rc = circkit_orfs_batch(c, s, offs, 1, &p, orf_offs, out, capacity, &total);
    if (count) *count = (size_t)total;
    return rc;
}

}  // extern "C"
