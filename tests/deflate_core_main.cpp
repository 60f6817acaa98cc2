// deflate_core_main.cpp — the host form of the BGZF deflate's core (cutesv_amd/csrc/deflate_core.h, DflOneLane) over a corpus file,
// as a stand-alone program: tests/test_bgzf_deflate.py builds it with -fsanitize=address,undefined.  Every input is a heap block
// of exactly its size, the token scratch has exactly one word per input byte, the output slot exactly the 65536 bytes of the
// contract: a byte read behind an input or written behind the slot is the sanitizer's to find.  The payload of every block is copied
// into a heap block of its own size and decoded again by inflate_core.h's host form in this program.
//
//   deflate_core_main CORPUS [OUT]  CORPUS: u32 count, then per block u32 bytes and the bytes; OUT: the BGZF blocks back to back
//   prints "limiter ok" (dfl_lengths on Fibonacci frequencies, limits 15 and 7), then per block:
//                                   index size stored fixed dynamic crc32-of-the-whole-block status-of-the-decode (0: the input came back)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../cutesv_amd/csrc/deflate_core.h"

static uint32_t rd32(FILE* f, bool* ok)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { *ok = false; return 0; }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

// dfl_lengths at its limit: Fibonacci frequencies - an unlimited Huffman tree over n of them is a chain of depth n - 1 - must come back
// with no length above maxbits, every symbol coded, and a complete code (Kraft sum exactly 1)
static bool limiter_ok(csv::DflWork* work, int n, int maxbits)
{
    uint32_t freq[288];
    uint8_t lens[288];
    uint32_t a = 1, b = 1;
    for (int s = 0; s < n; s++) { freq[s] = a; const uint32_t c = a + b; a = b; b = c; }
    memset(work, 0xA5, sizeof *work);
    memset(lens, 0xA5, sizeof lens);
    csv::dfl_lengths(csv::DflOneLane(), *work, freq, n, maxbits, lens, false);
    uint64_t kraft = 0;
    int longest = 0;
    for (int s = 0; s < n; s++) {
        if (lens[s] < 1 || lens[s] > maxbits) return false;
        if (s && lens[s] > lens[s - 1]) return false;              // a more frequent symbol never has the longer code
        kraft += 1ull << (maxbits - lens[s]);
        if (lens[s] > longest) longest = lens[s];
    }
    return kraft == 1ull << maxbits && longest == maxbits;
}

int main(int argc, char** argv)
{
    if (argc != 2 && argc != 3) { fprintf(stderr, "usage: %s CORPUS [OUT]\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    FILE* g = argc == 3 ? fopen(argv[2], "wb") : NULL;
    if (argc == 3 && !g) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    bool ok = true;
    const uint32_t n = rd32(f, &ok);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = csv::inf_crc_entry(i);
    csv::DflWork* work = (csv::DflWork*)malloc(sizeof(csv::DflWork));
    csv::InfWork* iwork = (csv::InfWork*)malloc(sizeof(csv::InfWork));
    if (!limiter_ok(work, 30, 15) || !limiter_ok(work, 22, 15) || !limiter_ok(work, 19, 7) || !limiter_ok(work, 17, 15)) { fprintf(stderr, "the length limiter fails on Fibonacci frequencies\n"); return 3; }
    printf("limiter ok\n");
    for (uint32_t k = 0; ok && k < n; k++) {
        const uint32_t len = rd32(f, &ok);
        if (!ok || len > (uint32_t)csv::DFL_MAX_IN) { ok = false; break; }
        uint8_t* in = (uint8_t*)malloc(len);
        if (len && fread(in, 1, len, f) != len) { ok = false; free(in); break; }
        uint32_t* tok = (uint32_t*)malloc(4 * (size_t)len);
        uint8_t* slot = (uint8_t*)malloc(csv::DFL_SLOT);
        memset(slot, 0xA5, csv::DFL_SLOT);
        memset(work, 0xA5, sizeof *work);                        // nothing an earlier block left helps this one
        int32_t sizes[3] = {0, 0, 0};
        const int32_t size = csv::dfl_block(csv::DflOneLane(), *work, in, (int32_t)len, tok, slot, table, sizes);
        int st = -1;
        uint32_t crc = 0;
        if (size >= 28 && size <= csv::DFL_SLOT) {
            crc = csv::InfOneLane().crc(slot, size, table);
            if (g && fwrite(slot, 1, (size_t)size, g) != (size_t)size) ok = false;
            const int32_t pn = size - 26;
            uint8_t* payload = (uint8_t*)malloc((size_t)pn);
            memcpy(payload, slot + 18, (size_t)pn);
            uint32_t want_crc = 0, isize = 0;
            for (int i = 0; i < 4; i++) { want_crc |= (uint32_t)slot[size - 8 + i] << (8 * i); isize |= (uint32_t)slot[size - 4 + i] << (8 * i); }
            uint8_t* back = (uint8_t*)malloc(len);
            st = isize == len ? 0 : 1000;
            if (!st && len) {
                memset(iwork, 0xA5, sizeof *iwork);
                st = csv::inf_block(csv::InfOneLane(), *iwork, payload, pn, back, (int32_t)len, want_crc, table);
                if (!st && memcmp(back, in, len) != 0) st = 2000;
            }
            free(back);
            free(payload);
        }
        printf("%u %d %d %d %d %u %d\n", k, size, sizes[0], sizes[1], sizes[2], crc, st);
        free(slot);
        free(tok);
        free(in);
    }
    free(iwork);
    free(work);
    fclose(f);
    if (g && fclose(g) != 0) ok = false;
    if (!ok) { fprintf(stderr, "%s: truncated or malformed corpus\n", argv[1]); return 2; }
    return 0;
}
