// Sanitizer driver of the offsets walk (test infrastructure; built by tests/test_csr_walk_cpu.py with
// g++ -fsanitize=address,undefined over circkit_amd/csrc/ck_csr.h -- CPU build only).
// Reads cases from argv[1]: u32 count, then per case {u64 limit, u64 n, (n + 1) x u64 offsets}.  Every offsets array is copied
// into a heap block of exactly its size, so a read past either end is an ASan report.  Writes per case to stdout:
// u32 fault (0 OK, 1 decrease, 2 too long), u64 index (~0 without a fault: the walk leaves it alone).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../circkit_amd/csrc/ck_csr.h"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t count = 0;
    if (fread(&count, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < count; ++k) {
        uint64_t head[2];
        if (fread(head, 8, 2, f) != 2) return 2;
        const uint64_t limit = head[0], n = head[1];
        uint64_t* offsets = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
        if (!offsets || fread(offsets, 8, n + 1, f) != n + 1) return 2;
        uint64_t at = ~0ull;
        const uint32_t fault = (uint32_t)ck_csr_walk(offsets, n, limit, &at);
        if (fwrite(&fault, 4, 1, stdout) != 1 || fwrite(&at, 8, 1, stdout) != 1) return 2;
        free(offsets);
    }
    fclose(f);
    return 0;
}
