// inflate_core_main.cpp — the host form of the BGZF inflate's decode core (cutesv_amd/csrc/inflate_core.h, InfOneLane) over a
// corpus file, as a stand-alone program: tests/test_bgzf_inflate.py builds it with -fsanitize=address,undefined and compares
// what it prints with zlib.  Every payload and every output lives in a heap block of exactly its size, so a byte read behind a
// payload or written behind out_len is the sanitizer's to find.
//
//   inflate_core_main CORPUS        CORPUS: u32 count, then per block u32 payload bytes, u32 isize, u32 crc, the payload
//   prints per block:               index status crc32-of-the-output adler32-of-the-output      (0 0 for a block with status != 0)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cutesv_amd/csrc/inflate_core.h"

static uint32_t rd32(FILE* f, bool* ok)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { *ok = false; return 0; }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    bool ok = true;
    const uint32_t n = rd32(f, &ok);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = csv::inf_crc_entry(i);
    csv::InfWork* work = (csv::InfWork*)malloc(sizeof(csv::InfWork));
    for (uint32_t k = 0; ok && k < n; k++) {
        const uint32_t in_len = rd32(f, &ok), isize = rd32(f, &ok), crc = rd32(f, &ok);
        if (!ok || in_len > (1u << 24) || isize > 65536u) { ok = false; break; }
        uint8_t* payload = (uint8_t*)malloc(in_len ? in_len : 1);
        if (in_len && fread(payload, 1, in_len, f) != in_len) { ok = false; free(payload); break; }
        if (!in_len) { free(payload); payload = (uint8_t*)malloc(0); }
        uint8_t* out = (uint8_t*)malloc(isize);
        int st = 0;
        if (isize) {                                             // (a block with out_len == 0 is skipped with status 0: the entry's rule)
            memset(out, 0xA5, isize);
            memset(work, 0xA5, sizeof *work);                    // no table entry of an earlier block helps this one
            st = csv::inf_block(csv::InfOneLane(), *work, payload, (int32_t)in_len, out, (int32_t)isize, crc, table);
        }
        uint32_t got = 0, a = 1, b = 0;
        if (!st) {
            got = isize ? csv::InfOneLane().crc(out, (int32_t)isize, table) : 0;
            for (uint32_t i = 0; i < isize; i++) { a = (a + out[i]) % 65521u; b = (b + a) % 65521u; }
        }
        printf("%u %d %u %u\n", k, st, st ? 0u : got, st ? 0u : (b << 16) | a);
        free(out);
        free(payload);
    }
    free(work);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: truncated or malformed corpus\n", argv[1]); return 2; }
    return 0;
}
