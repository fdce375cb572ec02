// orfs_lane_host.cpp -- TEST INFRASTRUCTURE ONLY: the per-lane routine of circkit_amd/csrc/orfs.h (orf_strand + sort_run)
// compiled for the host, so that tests/test_orfs_cpu.py can check the kernel's logic against the
// restatement (tests/orfs_ref.c) on a machine without a GPU.  A lane of orfs_count_kernel / orfs_emit_kernel touches
// nothing but its own record, so this is the kernel's computation, record for record.  Built by tests/orfs_ref.py.
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

#define __device__
#define __host__
#include "../circkit_amd/csrc/orfs.h"

using ck_orfs::Orf;

struct HostParams {                      // = tests/orfs_ref.c ref_params
    const uint8_t* start; int n_start;
    const uint8_t* stop; int n_stop;
    uint64_t min_length; double min_ratio;
    uint32_t min_wraps, max_wraps;
    int require_stop, strand_mask, mode;
};

extern "C" uint64_t ck_lane_orfs_batch(const uint8_t* bytes, const uint64_t* off, uint64_t n, const HostParams* p,
                                       uint64_t* out_off, Orf* out)
{
    uint8_t cls[512] = {};
    auto add = [&](const uint8_t* c, int k, uint8_t bit) {
        for (int i = 0; i < k; ++i) {
            uint32_t a = ck_orfs::sym_code(c[3 * i]), b = ck_orfs::sym_code(c[3 * i + 1]), d = ck_orfs::sym_code(c[3 * i + 2]);
            if (a == 6 || b == 6 || d == 6) continue;
            cls[(a << 6) | (b << 3) | d] |= bit;
        }
    };
    add(p->start, p->n_start, ck_orfs::CLS_START);
    add(p->stop, p->n_stop, ck_orfs::CLS_STOP);
    ck_orfs::Filter F{ p->min_length, p->min_ratio, p->min_wraps, p->max_wraps, (uint32_t)(p->require_stop != 0), (uint32_t)p->mode };
    out_off[0] = 0;
    std::vector<Orf> v;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* s = bytes + off[i];
        const uint64_t L = off[i + 1] - off[i];
        v.clear();
        if (L >= 2) {
            auto put = [&](const Orf& o) { v.push_back(o); };
            for (uint32_t st = 0; st < 2; ++st) {
                if (!(p->strand_mask & (1 << st))) continue;
                const size_t b = v.size();
                if (st == 0) ck_orfs::orf_strand<false>(s, (uint32_t)L, cls, F, 0, put);
                else ck_orfs::orf_strand<true>(s, (uint32_t)L, cls, F, 1, put);
                ck_orfs::sort_run(v.data() + b, (uint32_t)(v.size() - b), F.mode);      // the emit kernel's sort
            }
        }
        if (out) std::copy(v.begin(), v.end(), out + out_off[i]);
        out_off[i + 1] = out_off[i] + v.size();
    }
    return out_off[n];
}
