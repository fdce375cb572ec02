// circkit_hip.hip -- the ctx of include/circkit.h's C ABI: its lifecycle, its stream, and what the other units ask of it (ck_ctx.h).
// No device code: canonicalize is circkit_canon.hip, the benchmark helpers circkit_bench.hip, and every other unit a circkit_*.hip
// of its own that sees the ctx through ck_ctx.h.
// Built by __graft_entry__.build():  hipcc --offload-arch=gfx950 -O3 -shared -fPIC -> libcirckit_hip.so
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/circkit.h"
#include "fasta_host.h"
#include "ck_ctx_impl.h"

// the other units' view of the ctx (ck_ctx.h)
hipStream_t ck_ctx_stream(circkit_ctx* c) { return c->stream; }
int ck_ctx_device(circkit_ctx* c) { return c->device; }
const uint8_t* ck_ctx_complement(circkit_ctx* c) { return c->d_comp; }
void** ck_ctx_slot(circkit_ctx* c, ck_unit unit, void (*release)(void*)) { c->units[unit].release = release; return &c->units[unit].p; }
int ck_fail(circkit_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf;
    return code;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* circkit_version(void) { return "circkit-mi355x 0.1.0 (gfx950)"; }

int circkit_ctx_create(int device, circkit_ctx** out)
{
    if (!out) return CIRCKIT_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
        return CIRCKIT_ERR_NO_DEVICE;
    circkit_ctx* c = new circkit_ctx();
    c->device = device;
    *out = c;   // handed out even on failure below so the caller can read last_error, then destroy
    CK_HIP(c, hipSetDevice(device));
    CK_HIP(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    CK_HIP(c, hipEventCreate(&c->ev0));
    CK_HIP(c, hipEventCreate(&c->ev1));
    CK_HIP(c, hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
    int rc;
    if ((rc = c->h_mode.grow(c, 64, hipHostMallocMapped))) return rc;            // (canon_plan.h HostWord)
    c->h_mode[HM_MODE] = 0; c->h_mode[HM_TIERS] = 0;
    CK_HIP(c, hipHostGetDevicePointer((void**)&c->d_mode, (void*)c->h_mode.p, 0));
    if ((rc = c->d_comp.grow(c, 256)) || (rc = c->d_counters.grow(c, CTR_WORDS))) return rc;
    CK_HIP(c, hipMemset(c->d_counters, 0, CTR_WORDS * sizeof(uint32_t)));
    uint8_t comp[256];
    for (int v = 0; v < 256; ++v) comp[v] = (uint8_t)v;
    // bio 1.3.1 alphabets::dna complement table (call site lib/src/canonicalize.rs:56)
    const char *x = "AGCTYRWSKMDVHBN", *y = "TCGARYWSMKHBDVN";
    for (int i = 0; x[i]; ++i) { comp[(uint8_t)x[i]] = (uint8_t)y[i]; comp[(uint8_t)x[i] + 32] = (uint8_t)(y[i] + 32); }
    CK_HIP(c, hipMemcpy(c->d_comp, comp, 256, hipMemcpyHostToDevice));
    return ck_canon_init(c);
}

int circkit_ctx_destroy(circkit_ctx* c)
{
    if (!c) return CIRCKIT_OK;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->ev_head) (void)hipEventDestroy(c->ev_head);
    for (hipEvent_t e : c->ev_done) if (e) (void)hipEventDestroy(e);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    for (auto& u : c->units) if (u.release) u.release(u.p);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;                            // (with its buffers, device and page-locked)
    return CIRCKIT_OK;
}

const char* circkit_last_error(const circkit_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

// The ctx's lists, counters, hash flags and table are shared by everything it enqueues, and a caller may hand a later call
// tensors an earlier one has just written: work on the new stream must not overtake what is still queued on the old one.
// An event on the old stream, waited for by the new one -- no host-side wait; switching to the stream already bound costs
// nothing (circkit_amd/uniq.py rebinds before every table call).
static int switch_stream(circkit_ctx* c, hipStream_t s)
{
    if (s == c->stream) return CIRCKIT_OK;
    CK_HIP(c, hipSetDevice(c->device));
    // the stream being left may be gone already (an external stream its owner destroyed): the ordering then falls back to a
    // host-side wait for the device, and the ctx still moves -- it must not stay bound to a dead stream for good
    if (hipEventRecord(c->ev_order, c->stream) != hipSuccess || hipStreamWaitEvent(s, c->ev_order, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
        (void)hipGetLastError();
    }
    c->stream = s;
    return CIRCKIT_OK;
}

int circkit_ctx_set_stream(circkit_ctx* c, void* s)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    return switch_stream(c, (hipStream_t)s);      // NULL is a real stream: HIP's default (null) stream
}

int circkit_ctx_use_own_stream(circkit_ctx* c)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    return switch_stream(c, c->own_stream);
}

int circkit_ctx_synchronize(circkit_ctx* c)
{
    if (!c) return CIRCKIT_ERR_INVALID_ARG;
    CK_HIP(c, hipSetDevice(c->device));
    CK_HIP(c, hipStreamSynchronize(c->stream));
    return CIRCKIT_OK;
}

void* circkit_host_alloc(size_t bytes)
{
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void circkit_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

// needletail 0.5.1 sequence::normalize(seq, false) -- host logic of the CSR packer.
size_t circkit_normalize(const uint8_t* s, size_t n, uint8_t* out, int* changed)
{
    const uint8_t* lut = ckhost::normalize_lut();     // fasta_host.cpp: one table, built once (thread-safe)
    size_t m = 0; int ch = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t c = s[i], o = lut[c];
        ch |= (o != c);
        out[m] = o;
        m += (o != 0);
    }
    if (changed) *changed = ch;
    return m;
}

}  // extern "C"
