// CPU fiber run of the device FASTA writer (TEST INFRASTRUCTURE ONLY, never linked into the product): a stand-alone program that
// compiles circkit_amd/csrc/fasta_write.h against tests/emu/wave_prims_emu.h and links against libcanon_emu.so for the fiber
// scheduler.  It reads a file of cases and writes a file of results (formats: tests/emu/fasta_write_emu.py).  Per case the steps
// of circkit_fasta_write.hip run in their order: record_length() per record as the lengths kernel's lane runs it; the scan as
// plain host code with the same saturating sum (the scan kernels use no wave routine); verdict(); write_tile() as a workgroup of
// the product's WRITE_WAVES waves per output tile, so a lane that skips a collective deadlocks its wave, and UBSan + bounds
// checks watch every shift and access.  The text, the body and the output each lie in an exactly sized heap block between
// canaries; every input array is compared with its copy afterwards.  An output may be placed inside (or next to) the text's or
// the body's block, for the overlap verdict: then everything in that block but the accepted output must be unchanged.
//   fasta_write_emu_main --constants          prints "TILE_BYTES WRITE_WAVES SCAN_TILE SCAN_WG"
//   fasta_write_emu_main CASES RESULTS
#define CK_WAVE_PRIMS_OVERRIDE "../../tests/emu/wave_prims_emu.h"      // (relative to circkit_amd/csrc/wave_prims.h)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../circkit_amd/csrc/wave_prims.h"

namespace ck { namespace emu {
void run_block(void (*body)(void*), void* arg, int nwaves);            // tests/emu/emu.cpp
}}

#include "../../circkit_amd/csrc/fasta_write.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t IN_CANARY = 0x4E, OUT_CANARY = 0x3F;
enum { RC_OK = 0, RC_LANES_DISAGREE = 1, RC_CANARY = 2 };
enum { HAS_SRC = 1, HAS_LABELS = 2, HAS_BODY = 4 };
enum { ALIAS_NONE, ALIAS_TEXT, ALIAS_BODY };

struct Launch {
    ck_fwrite::Write W;
    uint64_t tile;
    uint64_t first[ck_fwrite::WRITE_WAVES][64];
};
void body(void* p)
{
    Launch* L = (Launch*)p;
    ck_fwrite::write_tile(L->W, L->tile, &L->first[ck::wave_in_block()][ck::lane_id()]);
}

// a block whose byte `shift` + `room` past a 64-byte boundary is the first of `size` bytes of use; `room` more bytes on either
// side of them (for an output placed next to them), then GUARD canary bytes on either side
struct Block {
    uint8_t* raw = nullptr;
    size_t shift, room, size, whole;
    Block(size_t shift_, size_t room_, size_t size_, uint8_t canary) : shift(shift_), room(room_), size(size_)
    {
        whole = GUARD + shift + room + size + room + GUARD;
        if (posix_memalign((void**)&raw, 64, whole)) abort();
        memset(raw, canary, whole);
    }
    ~Block() { free(raw); }
    uint8_t* use() { return raw + GUARD + shift + room; }
};

bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("write"); exit(3); } }

bool differ(const void* a, const void* b, size_t n) { return n != 0 && memcmp(a, b, n) != 0; }

// the block equals its snapshot everywhere but in [skip, skip + skip_n)
bool unchanged(const Block& b, const std::vector<uint8_t>& snap, const uint8_t* skip, size_t skip_n)
{
    for (size_t i = 0; i < b.whole; ++i) {
        const uint8_t* at = b.raw + i;
        if (skip_n && at >= skip && at < skip + skip_n) continue;
        if (*at != snap[i]) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "--constants")) {
        printf("%u %u %u %u\n", ck_fwrite::TILE_BYTES, ck_fwrite::WRITE_WAVES, ck_fwrite::SCAN_TILE, ck_fwrite::SCAN_WG);
        return 0;
    }
    if (argc != 3) { fprintf(stderr, "usage: %s CASES RESULTS | --constants\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { perror("open"); return 2; }

    uint64_t n_cases = 0;
    if (!get(in, &n_cases, 8)) return 2;
    for (uint64_t c = 0; c < n_cases; ++c) {
        // n_text, n_heads, n_src, flags, n_out, body bytes, text_shift, body_shift, out_shift, capacity (~0: the total), alias, alias_at
        uint64_t h[12];
        if (!get(in, h, sizeof h)) { fprintf(stderr, "case %llu: short header\n", (unsigned long long)c); return 2; }
        const uint64_t n_text = h[0], n_heads = h[1], n_src = h[2], flags = h[3], m = h[4], nb = h[5], alias = h[10];
        const int64_t alias_at = (int64_t)h[11];
        const bool has_src = flags & HAS_SRC, has_labels = flags & HAS_LABELS, has_body = flags & HAS_BODY;
        std::vector<uint8_t> text_in(n_text), body_in(has_body ? nb : 0);
        std::vector<ck_fwrite::Span> head(n_heads), raw(has_body ? 0 : n_heads);
        std::vector<uint64_t> src(has_src ? n_src : 0), body_off(has_body ? m + 1 : 0), out_offsets(m + 1);
        std::vector<ck_fwrite::Label> labels(has_labels ? m : 0);
        if (!get(in, text_in.data(), n_text) || !get(in, head.data(), 16 * head.size()) || !get(in, raw.data(), 16 * raw.size()) ||
            !get(in, src.data(), 8 * src.size()) || !get(in, labels.data(), sizeof(ck_fwrite::Label) * labels.size()) ||
            !get(in, body_off.data(), 8 * body_off.size()) || !get(in, body_in.data(), body_in.size())) {
            fprintf(stderr, "case %llu: short body\n", (unsigned long long)c);
            return 2;
        }
        const std::vector<ck_fwrite::Span> head_before = head, raw_before = raw;
        const std::vector<uint64_t> src_before = src, body_off_before = body_off;
        const std::vector<ck_fwrite::Label> labels_before = labels;

        // the lengths and their scan read no text and no body: the blocks are sized once the total is known
        ck_fwrite::Source S;
        S.text = nullptr; S.n_text = n_text;
        S.head = head.data(); S.raw = has_body ? nullptr : raw.data(); S.n_heads = n_heads;
        S.src = has_src ? src.data() : nullptr; S.n_src = n_src;
        S.labels = has_labels ? labels.data() : nullptr;
        S.body = has_body ? (const uint8_t*)1 : nullptr;           // (non-null: the lengths only ask whether there is one)
        S.body_offsets = has_body ? body_off.data() : nullptr;
        S.b0 = has_body && m ? body_off[0] : 0;
        S.b1 = has_body && m ? body_off[m] : 0;
        uint64_t n_invalid = 0, total = 0;
        out_offsets[0] = 0;
        for (uint64_t k = 0; k < m; ++k) {
            bool invalid;
            total = ck_fwrite::sat_add(total, ck_fwrite::record_length(S, k, &invalid));
            out_offsets[k + 1] = total;
            n_invalid += invalid;
        }
        const uint64_t capacity = h[9] == ~0ull ? total : h[9];
        const uint64_t fits = total > capacity || total == ~0ull ? 0 : total;      // the bytes an accepted write stores
        const size_t room = alias ? (size_t)fits + 48 : 0;
        Block text(h[6], alias == ALIAS_TEXT ? room : 0, n_text, IN_CANARY), bodyb(h[7], alias == ALIAS_BODY ? room : 0, body_in.size(), IN_CANARY);
        Block output(h[8], 0, alias ? 0 : (size_t)capacity, OUT_CANARY);
        if (n_text) memcpy(text.use(), text_in.data(), n_text);
        if (!body_in.empty()) memcpy(bodyb.use(), body_in.data(), body_in.size());
        uint8_t* dst = alias == ALIAS_TEXT ? text.use() + alias_at : alias == ALIAS_BODY ? bodyb.use() + S.b0 + alias_at : output.use();
        const std::vector<uint8_t> text_snap(text.raw, text.raw + text.whole), body_snap(bodyb.raw, bodyb.raw + bodyb.whole),
            out_snap(output.raw, output.raw + output.whole);
        S.text = text.use();
        if (has_body) S.body = bodyb.use();
        const uint64_t refused = ck_fwrite::verdict(total, capacity, S.text, n_text, S.body, S.b0, S.b1, dst);

        uint64_t rc = RC_OK;
        if (!refused && total) {
            Launch* L = new Launch();
            L->W.S = S;
            L->W.out_offsets = out_offsets.data();
            L->W.m = m; L->W.B = total;
            L->W.out = dst;
            const uint64_t n_gran = (((uint64_t)(uintptr_t)dst & 15u) + total + 15) / 16;
            const uint64_t n_tiles = (n_gran + ck_fwrite::TILE_GRANULES - 1) / ck_fwrite::TILE_GRANULES;
            for (uint64_t t = 0; t < n_tiles && rc == RC_OK; ++t) {
                L->tile = t;
                for (auto& wv : L->first) for (uint64_t& v : wv) v = ~0ull;
                ck::emu::run_block(body, L, (int)ck_fwrite::WRITE_WAVES);
                for (auto& wv : L->first)
                    for (int l = 1; l < 64; ++l) if (wv[l] != wv[0]) rc = RC_LANES_DISAGREE;
            }
            delete L;
        }
        const uint64_t written = refused ? 0 : total;
        if (!unchanged(text, text_snap, dst, written) || !unchanged(bodyb, body_snap, dst, written) || !unchanged(output, out_snap, dst, written) ||
            differ(head_before.data(), head.data(), 16 * head.size()) || differ(raw_before.data(), raw.data(), 16 * raw.size()) ||
            differ(src_before.data(), src.data(), 8 * src.size()) || differ(body_off_before.data(), body_off.data(), 8 * body_off.size()) ||
            differ(labels_before.data(), labels.data(), sizeof(ck_fwrite::Label) * labels.size()))
            rc = rc ? rc : RC_CANARY;
        const uint64_t r[4] = { rc, total, n_invalid, refused };
        put(out, r, sizeof r);
        put(out, out_offsets.data(), 8 * (m + 1));
        put(out, dst, written);
    }
    if (fclose(out)) { perror("close"); return 3; }
    fclose(in);
    return 0;
}
