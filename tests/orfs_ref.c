/*
 * orfs_ref.c -- TEST INFRASTRUCTURE ONLY: a literal C restatement of the reference's ORF finder, the checker the GPU
 * kernels of circkit_amd/csrc/orfs.h are compared against.  Built by tests/orfs_ref.py (gcc, when stale) and by
 * __graft_entry__.build().
 *
 * Restated (paths relative to the reference checkout):
 *   lib/src/orfs.rs:57-70    add_last_codons                          -> add_last_codons()
 *   lib/src/orfs.rs:73-93    start_stop_codon_indices_by_frame_naive  -> indices_by_frame()
 *   lib/src/orfs.rs:149-298  find_orfs_with_indices                   -> find_orfs_with_indices()
 *   lib/src/orfs.rs:301-315  longest_orfs                             -> longest_orfs()
 *   src/orfs.rs:53-104       the worker closure: normalize is the caller's (the batch holds normalized records),
 *                            filter, longest, and the reverse strand on bio's revcomp of the record.
 * Per-frame index lists are kept as the reference keeps them (ascending, wrap codons appended last), and the `find`
 * calls scan them in the same order.
 */
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
    uint64_t length;
    uint32_t start, stop, wraps, strand;   /* stop == UINT32_MAX: None */
} ref_orf;

typedef struct {
    const uint8_t *codons; int n;          /* n codons of 3 bytes each */
} codon_set;

typedef struct {
    codon_set start, stop;
    uint64_t min_length; double min_ratio;
    uint32_t min_wraps, max_wraps;
    int require_stop, strand_mask, mode;   /* strand_mask: 1 forward, 2 reverse; mode 0 = longest per stop, 1 = all (find order) */
} ref_params;

#define NONE UINT32_MAX

typedef struct { uint32_t *v; size_t n; } ivec;

static int contains(const codon_set *s, const uint8_t c[3])
{
    for (int i = 0; i < s->n; ++i)
        if (s->codons[3 * i] == c[0] && s->codons[3 * i + 1] == c[1] && s->codons[3 * i + 2] == c[2]) return 1;
    return 0;
}

/* lib/src/orfs.rs:57-70 */
static void add_last_codons(const uint8_t *seq, size_t L, const codon_set *codons, ivec by_frame[3])
{
    uint8_t pen[3] = { seq[L - 2], seq[L - 1], seq[0] };
    if (contains(codons, pen)) { ivec *f = &by_frame[(L - 2) % 3]; f->v[f->n++] = (uint32_t)(L - 2); }
    uint8_t ult[3] = { seq[L - 1], seq[0], seq[1] };
    if (contains(codons, ult)) { ivec *f = &by_frame[(L - 1) % 3]; f->v[f->n++] = (uint32_t)(L - 1); }
}

/* lib/src/orfs.rs:73-93 (L >= 2) */
static void indices_by_frame(const uint8_t *seq, size_t L, const ref_params *p, ivec starts[3], ivec stops[3])
{
    for (size_t i = 0; i + 2 < L; ++i) {
        if (contains(&p->start, seq + i)) { ivec *f = &starts[i % 3]; f->v[f->n++] = (uint32_t)i; }
        else if (contains(&p->stop, seq + i)) { ivec *f = &stops[i % 3]; f->v[f->n++] = (uint32_t)i; }
    }
    add_last_codons(seq, L, &p->start, starts);
    add_last_codons(seq, L, &p->stop, stops);
}

static void push(ref_orf **out, size_t *n, size_t *cap, uint32_t start, uint32_t stop, uint32_t wraps, uint64_t length)
{
    if (*n == *cap) { *cap = *cap ? 2 * *cap : 64; *out = (ref_orf *)realloc(*out, *cap * sizeof(ref_orf)); }
    (*out)[(*n)++] = (ref_orf){ length, start, stop, wraps, 0 };
}

/* lib/src/orfs.rs:149-298 */
static void find_orfs_with_indices(size_t seq_len, ivec starts[3], ivec stops[3], ref_orf **out, size_t *n, size_t *cap)
{
    for (int fr = 0; fr < 3; ++fr)                               /* .iter().flatten() */
        for (size_t k = 0; k < starts[fr].n; ++k) {
            uint32_t s = starts[fr].v[k];
            size_t cur = s % 3;
            uint64_t orf_length = 0;
            if (seq_len % 3 == 0) {
                uint32_t stop = NONE;
                for (size_t j = 0; j < stops[cur].n; ++j) if (stops[cur].v[j] > s) { stop = stops[cur].v[j]; break; }
                if (stop == NONE)
                    for (size_t j = 0; j < stops[cur].n; ++j) if (stops[cur].v[j] < s) { stop = stops[cur].v[j]; break; }
                /* `stop_codon_index < Some(start)` is true for None */
                uint32_t wraps = (stop == NONE || stop < s || (seq_len - stop < 3)) ? 1 : 0;
                uint64_t length = stop == NONE ? seq_len : (stop >= s ? (uint64_t)stop - s + 3 : (uint64_t)stop + seq_len - s + 3);
                push(out, n, cap, s, stop, wraps, length);
                continue;
            }
            uint32_t stop = NONE;
            for (size_t j = 0; j < stops[cur].n; ++j) if (stops[cur].v[j] >= s) { stop = stops[cur].v[j]; break; }
            if (stop != NONE) {
                push(out, n, cap, s, stop, seq_len - stop >= 3 ? 0 : 1, (uint64_t)stop - s + 3);
                continue;
            }
            orf_length += seq_len - s;
            cur = seq_len % 3 == 2 ? (cur + 1) % 3 : (cur + 2) % 3;
            if (stops[cur].n) {
                uint32_t st = stops[cur].v[0];
                push(out, n, cap, s, st, seq_len - st >= 3 ? 1 : 2, orf_length + st + 3);
                continue;
            }
            orf_length += seq_len;
            cur = seq_len % 3 == 2 ? (cur + 1) % 3 : (cur + 2) % 3;
            if (stops[cur].n) {
                uint32_t st = stops[cur].v[0];
                push(out, n, cap, s, st, seq_len - st >= 3 ? 2 : 3, orf_length + st + 3);
                continue;
            }
            orf_length += seq_len;
            cur = seq_len % 3 == 2 ? (cur + 1) % 3 : (cur + 2) % 3;
            if (stops[cur].n) {
                uint32_t st = stops[cur].v[0];
                push(out, n, cap, s, st, 3, orf_length + st + 3);
                continue;
            }
            orf_length += s;
            push(out, n, cap, s, NONE, 3, orf_length);
        }
}

/* stable sort by length ascending (merge sort: Vec::sort_by_key is stable) */
static void stable_sort_by_length(ref_orf *a, size_t n, ref_orf *tmp)
{
    if (n < 2) return;
    size_t h = n / 2;
    stable_sort_by_length(a, h, tmp);
    stable_sort_by_length(a + h, n - h, tmp);
    size_t i = 0, j = h, k = 0;
    while (i < h && j < n) tmp[k++] = a[j].length < a[i].length ? a[j++] : a[i++];
    while (i < h) tmp[k++] = a[i++];
    while (j < n) tmp[k++] = a[j++];
    memcpy(a, tmp, n * sizeof(ref_orf));
}

/* lib/src/orfs.rs:301-315; returns the kept count, kept ORFs moved to the front of a */
static size_t longest_orfs(ref_orf *a, size_t n, size_t seq_len)
{
    ref_orf *tmp = (ref_orf *)malloc((n ? n : 1) * sizeof(ref_orf));
    stable_sort_by_length(a, n, tmp);
    for (size_t i = 0; i < n / 2; ++i) { ref_orf t = a[i]; a[i] = a[n - 1 - i]; a[n - 1 - i] = t; }
    uint8_t *seen = (uint8_t *)calloc(seq_len + 1, 1);          /* [seq_len] = the None key */
    size_t m = 0;
    for (size_t i = 0; i < n; ++i) {
        size_t key = a[i].stop == NONE ? seq_len : a[i].stop;
        if (!seen[key]) { seen[key] = 1; a[m++] = a[i]; }
    }
    free(seen); free(tmp);
    return m;
}

/* bio 1.3.1 alphabets::dna complement */
static uint8_t g_comp[256];
static void comp_init(void)
{
    for (int v = 0; v < 256; ++v) g_comp[v] = (uint8_t)v;
    const char *a = "AGCTYRWSKMDVHBN", *b = "TCGARYWSMKHBDVN";
    for (int i = 0; a[i]; ++i) {
        g_comp[(uint8_t)a[i]] = (uint8_t)b[i];
        g_comp[(uint8_t)a[i] + 32] = (uint8_t)(b[i] + 32);
    }
}

/* one strand of the worker closure (src/orfs.rs:61-81 / :83-100) */
static size_t one_strand(const uint8_t *seq, size_t L, const ref_params *p, uint32_t strand, ref_orf **out, size_t *n, size_t *cap)
{
    ivec starts[3], stops[3];
    for (int f = 0; f < 3; ++f) {
        starts[f].v = (uint32_t *)malloc((L / 3 + 2) * sizeof(uint32_t)); starts[f].n = 0;
        stops[f].v = (uint32_t *)malloc((L / 3 + 2) * sizeof(uint32_t)); stops[f].n = 0;
    }
    indices_by_frame(seq, L, p, starts, stops);
    size_t base = *n;
    find_orfs_with_indices(L, starts, stops, out, n, cap);
    size_t m = base;
    for (size_t i = base; i < *n; ++i) {                                 /* all_orfs.retain(..) */
        ref_orf o = (*out)[i];
        if (o.length - 3 >= p->min_length && (!p->require_stop || o.stop != NONE) && p->min_wraps <= o.wraps &&
            o.wraps <= p->max_wraps && (double)o.length / (double)L >= p->min_ratio)
            (*out)[m++] = o;
    }
    *n = m;
    if (p->mode == 0) *n = base + longest_orfs(*out + base, *n - base, L);
    for (size_t i = base; i < *n; ++i) (*out)[i].strand = strand;
    for (int f = 0; f < 3; ++f) { free(starts[f].v); free(stops[f].v); }
    return *n - base;
}

/* Every ORF of one normalized record: forward strand, then reverse, per strand_mask.  Records of fewer than 2 symbols
 * (a panic in the reference) give none.  *out is realloc'ed; returns the count. */
size_t ck_ref_orfs_record(const uint8_t *seq, size_t L, const ref_params *p, ref_orf **out, size_t *cap)
{
    size_t n = 0;
    if (L < 2) return 0;
    if (p->strand_mask & 1) one_strand(seq, L, p, 0, out, &n, cap);
    if (p->strand_mask & 2) {
        uint8_t *rc = (uint8_t *)malloc(L);
        for (size_t i = 0; i < L; ++i) rc[i] = g_comp[seq[L - 1 - i]];
        one_strand(rc, L, p, 1, out, &n, cap);
        free(rc);
    }
    return n;
}

/* lib/src/orfs.rs:41 find_orfs (ATG / TAA,TAG,TGA, no filter, no longest step).  The Aho-Corasick scan of the
 * reference finds the same indices as the naive one for these non-overlapping sets (its own proptest :656-665). */
size_t ck_ref_find_orfs(const uint8_t *seq, size_t L, ref_orf *out, size_t cap)
{
    static const uint8_t st[] = "ATG", sp[] = "TAATAGTGA";
    ref_params p = { { st, 1 }, { sp, 3 }, 0, 0.0, 0, 3, 0, 1, 1 };
    ref_orf *v = NULL; size_t vc = 0;
    size_t n = ck_ref_orfs_record(seq, L, &p, &v, &vc);
    memcpy(out, v, (n < cap ? n : cap) * sizeof(ref_orf));
    free(v);
    return n;
}

typedef struct {
    const uint8_t *bytes; const uint64_t *off; const ref_params *p;
    uint64_t lo, hi; uint64_t *counts; ref_orf *out; const uint64_t *out_off;
} job_t;

static void *worker(void *arg)
{
    job_t *j = (job_t *)arg;
    ref_orf *v = NULL; size_t vc = 0;
    for (uint64_t i = j->lo; i < j->hi; ++i) {
        size_t n = ck_ref_orfs_record(j->bytes + j->off[i], j->off[i + 1] - j->off[i], j->p, &v, &vc);
        if (j->out) memcpy(j->out + j->out_off[i], v, n * sizeof(ref_orf));
        else j->counts[i] = n;
    }
    free(v);
    return NULL;
}

static void run(job_t proto, uint64_t n, int threads)
{
    if (threads < 1) threads = 1;
    pthread_t th[256]; job_t jobs[256];
    if (threads > 256) threads = 256;
    for (int t = 0; t < threads; ++t) {
        jobs[t] = proto;
        jobs[t].lo = n * t / threads; jobs[t].hi = n * (t + 1) / threads;
        pthread_create(&th[t], NULL, worker, &jobs[t]);
    }
    for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
}

/* CSR batch: out_off[n + 1] (exclusive scan of the per-record counts, out_off[0] = 0) always; out (nullable) gets
 * every record's ORFs in record order.  Two passes over the records on `threads` threads. */
uint64_t ck_ref_orfs_batch(const uint8_t *bytes, const uint64_t *off, uint64_t n, const ref_params *p, uint64_t *out_off,
                           ref_orf *out, int threads)
{
    comp_init();
    job_t j = { bytes, off, p, 0, 0, out_off + 1, NULL, NULL };
    run(j, n, threads);
    out_off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) out_off[i + 1] += out_off[i];
    if (out) {
        j.counts = NULL; j.out = out; j.out_off = out_off;
        run(j, n, threads);
    }
    return out_off[n];
}

void ck_ref_init(void) { comp_init(); }
