// prims_probe.hip -- the op table of tests/prims/prims_ops.h against the gfx950 device half of circkit_amd/csrc/wave_prims.h
// (TEST INFRASTRUCTURE ONLY: tests/prims_probe.py builds it into tests/libck_prims_probe.so, never part of the product library).
// One workgroup per case, every wave of the workgroup runs the case: wave w of case c reads the case's inputs, writes the
// results of its own (out + (c * nwaves + w) * 64 * OUT_W) and has global memory of its own (pool + (mem * nwaves + w) * MEM_BYTES,
// mem = the case's slot; slot 0 belongs to the cases that touch none).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../circkit_amd/csrc/wave_prims.h"
#include "prims_ops.h"

namespace {

__global__ void __launch_bounds__(1024) prims_probe_kernel(const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                           uint8_t* pool, uint32_t n_cases)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[16 * ck_prims::LDS_DW];
    __shared__ uint32_t xchg[ck_prims::XCHG_DW];
    const uint32_t c = blockIdx.x;
    if (c >= n_cases) return;
    const uint32_t w = ck::wave_in_block(), t = ck::lane_id(), nwaves = blockDim.x >> 6;
    const uint32_t op = ck::uniform(hdr[4 * c]), mode = ck::uniform(hdr[4 * c + 1]), mem = ck::uniform(hdr[4 * c + 2]);
    uint8_t* g = pool + ((uint64_t)mem * nwaves + w) * ck_prims::MEM_BYTES;
    const uint32_t* li = in + ((uint64_t)c * 64 + t) * ck_prims::IN_W;
    uint32_t* lo = out + (((uint64_t)c * nwaves + w) * 64 + t) * ck_prims::OUT_W;
    uint32_t* lds = lds_all + w * ck_prims::LDS_DW;
    if (mode) ck_prims::run_case<1>(op, li, lo, g, lds, xchg, nwaves);
    else ck_prims::run_case<0>(op, li, lo, g, lds, xchg, nwaves);
}

}  // namespace

// device pointers; threads = 64 .. 1024, a multiple of 64.  Returns the HIP error of the launch (0: none); the caller synchronizes.
extern "C" int ck_prims_probe_launch(const void* hdr, const void* in, void* out, void* pool, uint32_t n_cases, uint32_t threads, void* stream)
{
    if (threads < 64 || threads > 1024 || threads % 64) return -1;
    if (n_cases == 0) return 0;
    hipLaunchKernelGGL(prims_probe_kernel, dim3(n_cases), dim3(threads), 0, (hipStream_t)stream, (const uint32_t*)hdr, (const uint32_t*)in,
                       (uint32_t*)out, (uint8_t*)pool, n_cases);
    return (int)hipGetLastError();
}
