/* mono_ref.c -- TEST INFRASTRUCTURE ONLY: a literal restatement of the reference's Monomerizer
 * (lib/src/monomerize.rs:43-135), written from its behaviour.  The GPU kernel and its CPU emulation are checked against this.
 *
 *   first    first_monomer_end_index: the seed is the last k bytes; a plain ascending search finds its occurrences in the
 *            text before it (ShiftAnd::find_all yields the same start positions in the same order); the first one whose
 *            overlap passes ends the pass
 *   last     last_monomer_end_index: the pass repeated on the shrinking prefix
 *   sens     last_monomer_end_index_sensitive through an ACTUAL reverse complement with the table the caller sets
 *            (ck_mono_ref_set_complement: the oracle's table, bio's dna::complement)
 *   free     the same without the complement (the form the kernel uses), so that a test can compare the two
 *
 * Every function adds the bytes it compares (searched text + overlap bytes) to *work when work is given. */
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint32_t seed_len;
    uint32_t use_identity;
    uint64_t overlap_dist;
    double min_identity;
    uint32_t sensitive;
} ck_mono_ref_params;

static uint8_t g_comp[256];

void ck_mono_ref_set_complement(const uint8_t* table) { memcpy(g_comp, table, 256); }

static uint64_t max_dist_of(const ck_mono_ref_params* P, size_t ovl)
{
    if (!P->use_identity) return P->overlap_dist;
    volatile double prod = (double)ovl * P->min_identity;       /* one rounded f64 product */
    return (uint64_t)ovl - (uint64_t)floor(prod);
}

/* -1 = None */
int64_t ck_mono_ref_first(const uint8_t* s, size_t m, const ck_mono_ref_params* P, uint64_t* work)
{
    const size_t k = P->seed_len;
    if (m <= k) return -1;
    const uint8_t* seed = s + (m - k);
    const size_t text = m - k;
    if (work) *work += text;
    for (size_t occ = 0; occ + k <= text; ++occ) {
        if (memcmp(s + occ, seed, k) != 0) continue;
        const size_t ovl = occ + k;
        const uint8_t* starter = s + (m - ovl);
        uint64_t dist = 0;
        for (size_t i = 0; i < ovl; ++i) dist += s[i] != starter[i];
        if (work) *work += ovl;
        if (dist <= max_dist_of(P, ovl)) return (int64_t)(m - ovl);
    }
    return -1;
}

int64_t ck_mono_ref_last(const uint8_t* s, size_t n, const ck_mono_ref_params* P, uint64_t* work)
{
    int64_t res = ck_mono_ref_first(s, n, P, work);
    while (res >= 0) {
        const int64_t nxt = ck_mono_ref_first(s, (size_t)res, P, work);
        if (nxt < 0) break;
        res = nxt;
    }
    return res;
}

int64_t ck_mono_ref_sensitive(const uint8_t* s, size_t n, const ck_mono_ref_params* P, uint64_t* work)
{
    const int64_t idx = ck_mono_ref_last(s, n, P, work);
    const size_t M = idx >= 0 ? (size_t)idx : n;
    uint8_t* rc = (uint8_t*)malloc(M ? M : 1);
    for (size_t i = 0; i < M; ++i) rc[i] = g_comp[s[M - 1 - i]];
    const int64_t r = ck_mono_ref_first(rc, M, P, work);
    free(rc);
    if (r < 0) return idx;
    return (int64_t)(M - (M - (size_t)r));
}

/* the sensitive form without a complement: the largest q in [k, M - k] with s[q..q+k) == s[0..k) whose overlap passes */
int64_t ck_mono_ref_sensitive_free(const uint8_t* s, size_t n, const ck_mono_ref_params* P)
{
    const int64_t idx = ck_mono_ref_last(s, n, P, NULL);
    const size_t M = idx >= 0 ? (size_t)idx : n, k = P->seed_len;
    if (M < 2 * k) return idx;
    for (size_t q = M - k;; --q) {
        if (memcmp(s + q, s, k) == 0) {
            const size_t ovl = M - q;
            uint64_t dist = 0;
            for (size_t i = 0; i < ovl; ++i) dist += s[i] != s[q + i];
            if (dist <= max_dist_of(P, ovl)) return (int64_t)q;
        }
        if (q == k) break;
    }
    return idx;
}

int64_t ck_mono_ref_end(const uint8_t* s, size_t n, const ck_mono_ref_params* P, uint64_t* work)
{
    return P->sensitive ? ck_mono_ref_sensitive(s, n, P, work) : ck_mono_ref_last(s, n, P, work);
}

/* ---- a batch on several threads: out[i] = the end index or 0xFFFFFFFF; returns the bytes compared ---- */
typedef struct {
    const uint8_t* bytes;
    const uint64_t* offsets;
    uint64_t n;
    const ck_mono_ref_params* P;
    uint32_t* out;
    uint64_t next, work;
    pthread_mutex_t mu;
} batch_job;

static void* batch_worker(void* arg)
{
    batch_job* J = (batch_job*)arg;
    uint64_t work = 0;
    for (;;) {
        const uint64_t a = __atomic_fetch_add(&J->next, 64, __ATOMIC_RELAXED);
        if (a >= J->n) break;
        const uint64_t b = a + 64 < J->n ? a + 64 : J->n;
        for (uint64_t i = a; i < b; ++i) {
            const int64_t r = ck_mono_ref_end(J->bytes + J->offsets[i], (size_t)(J->offsets[i + 1] - J->offsets[i]), J->P, &work);
            J->out[i] = r < 0 ? 0xFFFFFFFFu : (uint32_t)r;
        }
    }
    pthread_mutex_lock(&J->mu);
    J->work += work;
    pthread_mutex_unlock(&J->mu);
    return NULL;
}

uint64_t ck_mono_ref_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, const ck_mono_ref_params* P, uint32_t* out,
                           int threads)
{
    batch_job J;
    J.bytes = bytes; J.offsets = offsets; J.n = n; J.P = P; J.out = out; J.next = 0; J.work = 0;
    pthread_mutex_init(&J.mu, NULL);
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    pthread_t th[64];
    int started = 0;
    for (int t = 1; t < threads; ++t)
        if (pthread_create(&th[started], NULL, batch_worker, &J) == 0) ++started;
    batch_worker(&J);
    for (int t = 0; t < started; ++t) pthread_join(th[t], NULL);
    pthread_mutex_destroy(&J.mu);
    return J.work;
}
