// circkit_bench.hip -- the benchmark's helper kernels and their C ABI: synthetic bases, fixed-length offsets, the plain-copy yardstick.
// Nothing here is shared with the canonicalize path; the ctx is seen through ck_ctx.h.
#include <hip/hip_runtime.h>

#include "../../include/circkit.h"
#include "wave_prims.h"
#include "ck_ctx.h"

namespace {

constexpr int N_CU = 256;                                // (as in canon_config.h, by which the canonicalize unit sizes its own grids)

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// 16 bases per thread, 16-byte stores; base g uses bits 2*(g&31) of splitmix64(seed*K + (g>>5)).
__global__ __launch_bounds__(256) void synth_fill_kernel(uint64_t seed, uint64_t first_base, uint64_t n_bases,
                                                         uint8_t* out)
{
    const uint64_t key = seed * 0xD1342543DE82EF95ULL;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16;
    for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < n_bases; i += stride) {
        const uint64_t g0 = first_base + i;
        uint64_t wi = g0 >> 5, w = splitmix64(key + wi);
        uint32_t o[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const uint64_t g = g0 + b;
            if ((g >> 5) != wi) { wi = g >> 5; w = splitmix64(key + wi); }
            const uint32_t code = (uint32_t)(w >> (2 * (g & 31))) & 3u;
            o[b >> 2] |= ((0x54474341u >> (8 * code)) & 0xFFu) << (8 * (b & 3));
        }
        if (i + 16 <= n_bases) {
            ck::store16(out + i, ck::u32x4{ o[0], o[1], o[2], o[3] });
        } else {
            for (uint64_t b = 0; i + b < n_bases; ++b) out[i + b] = (uint8_t)(o[b >> 2] >> (8 * (b & 3)));
        }
    }
}

// Plain device-to-device copy, 16 bytes per lane, UNROLL loads in flight per lane: the same-process, same-box yardstick the
// bench line quotes next to the canonicalize kernel's rate (circkit_bench_copy_device; shapes from tools/microbench/ceiling_bench.hip).
typedef uint32_t copy_v4 __attribute__((ext_vector_type(4)));
template <int UNROLL>
__global__ __launch_bounds__(256) void bench_copy_kernel(const copy_v4* __restrict__ in, copy_v4* __restrict__ out, uint64_t n16)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256 * UNROLL;
    uint64_t i = (uint64_t)blockIdx.x * 256 * UNROLL + threadIdx.x;
    for (; i + 256 * (UNROLL - 1) < n16; i += stride) {
        copy_v4 r[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) r[u] = in[i + u * 256];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) out[i + u * 256] = r[u];
    }
    for (; i < n16; i += 256) out[i] = in[i];                 // the last, partial tile of the workgroup that owns it
}

__global__ void fixed_offsets_kernel(uint64_t base, uint64_t len, uint64_t n, uint64_t* off)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) off[i] = base + i * len;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int circkit_synth_fill_device(circkit_ctx* c, uint64_t seed, uint64_t first_base, uint64_t n_bases, uint8_t* d_bytes)
{
    if (!c || (n_bases && !d_bytes)) return CIRCKIT_ERR_INVALID_ARG;
    if (n_bases == 0) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    hipLaunchKernelGGL(synth_fill_kernel, dim3(N_CU * 8), dim3(256), 0, ck_ctx_stream(c), seed, first_base, n_bases, d_bytes);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

int circkit_fixed_offsets_device(circkit_ctx* c, uint64_t base, uint64_t len, uint64_t n, uint64_t* d_offsets)
{
    if (!c || !d_offsets) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    hipLaunchKernelGGL(fixed_offsets_kernel, dim3(N_CU * 4), dim3(256), 0, ck_ctx_stream(c), base, len, n, d_offsets);
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

// Measurement helper: enqueues one plain copy of `bytes` bytes (rounded down to 16) on the ctx stream.
int circkit_bench_copy_device(circkit_ctx* c, const void* d_src, void* d_dst, uint64_t bytes, uint32_t variant)
{
    if (!c || !d_src || !d_dst || variant >= 5) return CIRCKIT_ERR_INVALID_ARG;
    if (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) return ck_fail(c, CIRCKIT_ERR_INVALID_ARG, "circkit_bench_copy_device: 16-byte aligned buffers");
    CK_HIP(c, hipSetDevice(ck_ctx_device(c)));
    const uint64_t n16 = bytes / 16;
    const copy_v4* in = (const copy_v4*)d_src; copy_v4* out = (copy_v4*)d_dst;
    switch (variant) {
    case 0: hipLaunchKernelGGL(bench_copy_kernel<4>, dim3(2048), dim3(256), 0, ck_ctx_stream(c), in, out, n16); break;
    case 1: hipLaunchKernelGGL(bench_copy_kernel<8>, dim3(2048), dim3(256), 0, ck_ctx_stream(c), in, out, n16); break;
    case 2: hipLaunchKernelGGL(bench_copy_kernel<4>, dim3(8192), dim3(256), 0, ck_ctx_stream(c), in, out, n16); break;
    case 3: hipLaunchKernelGGL(bench_copy_kernel<2>, dim3(65536), dim3(256), 0, ck_ctx_stream(c), in, out, n16); break;
    default: CK_HIP(c, hipMemcpyAsync(d_dst, d_src, n16 * 16, hipMemcpyDeviceToDevice, ck_ctx_stream(c))); break;      // the runtime's own copy
    }
    CK_HIP(c, hipGetLastError());
    return CIRCKIT_OK;
}

}  // extern "C"
