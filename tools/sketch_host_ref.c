/* One-thread restatement of the sketch definition of include/circkit.h ("sketches of circular records") for
 * tools/bench_sketch.py: the figure circkit_sketch_batch from page-locked host buffers is held against, and a third opinion on
 * its rows.  Not part of the product and not the tests' yardstick (tests/sketch_ref.py).  The k-mers roll: one shift per symbol
 * for the forward packing and one for the reverse complement, `good` = the ACGT symbols since the last other byte. */
#include <stdint.h>

static uint64_t fmix64(uint64_t h)
{
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

static int code_of(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : -1; }

void sketch_host(const uint8_t* bytes, const uint64_t* offsets, uint64_t n_records, uint32_t k, uint32_t log2_bins, uint64_t seed, uint64_t* out,
                 uint32_t* counts)
{
    const uint64_t bins = 1ull << log2_bins, mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
    for (uint64_t i = 0; i < n_records; ++i) {
        const uint8_t* s = bytes + offsets[i];
        const uint64_t n = offsets[i + 1] - offsets[i];
        uint64_t* row = out + i * bins;
        uint32_t count = 0;
        for (uint64_t b = 0; b < bins; ++b) row[b] = ~0ull;
        if (n >= k) {
            uint64_t f = 0, r = 0, good = 0, at = 0;
            for (uint64_t j = 0; j < n + k - 1; ++j) {           /* symbol j mod n ends the k-mer that starts at j - k + 1 */
                const int c = code_of(s[at]);
                if (++at == n) at = 0;
                good = c < 0 ? 0 : good + 1;
                f = ((f << 2) | (uint64_t)(c < 0 ? 0 : c)) & mask;
                r = (r >> 2) | ((uint64_t)(c < 0 ? 0 : 3 - c) << (2 * k - 2));
                if (j + 1 >= k && good >= k) {
                    const uint64_t h = fmix64((f < r ? f : r) ^ seed);
                    uint64_t* bin = &row[h >> (64 - log2_bins)];
                    if (h < *bin) *bin = h;
                    ++count;
                }
            }
        }
        if (counts) counts[i] = count;
    }
}
