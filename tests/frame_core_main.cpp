// frame_core_main.cpp — the host form of the BAM framing core (cutesv_amd/csrc/frame_core.h, FrOneLane) over a corpus of windows,
// as a stand-alone program: tests/test_bam_frame.py builds it with -fsanitize=address,undefined and compares what it prints with
// its own chain walk.  Every window lives in a heap block of exactly its size, and so does every table the core writes, so a byte
// read behind a window or a start written behind a slot is the sanitizer's to find.  The program also walks the chain naively
// itself and fails when the core's record list differs.
//
//   frame_core_main CORPUS      CORPUS: u32 count, then per window: u32 bytes, i32 n_ref, u32 n_blocks, u32 c, u32 len[n_blocks], the bytes
//   prints per window:          index n_records tail tail_has_bs tail_bs right_blocks fallback_blocks fnv1a-of-the-rows
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../cutesv_amd/csrc/frame_core.h"

using csv::fr_i64;

static uint32_t rd32(FILE* f, bool* ok)
{
    uint8_t b[4];
    if (fread(b, 1, 4, f) != 4) { *ok = false; return 0; }
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

template <class T> static T* exact(size_t n) { return (T*)malloc(n * sizeof(T)); }      // (malloc(0) is a valid block of no bytes)

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    bool ok = true;
    const uint32_t n_win = rd32(f, &ok);
    int bad = 0;
    for (uint32_t k = 0; ok && k < n_win; k++) {
        const uint32_t nbytes = rd32(f, &ok);
        const int32_t n_ref = (int32_t)rd32(f, &ok);
        const uint32_t nb = rd32(f, &ok), c = rd32(f, &ok);
        if (!ok || nbytes > (1u << 28) || nb > (1u << 20)) { ok = false; break; }
        int32_t* len = exact<int32_t>(nb);
        fr_i64* off = exact<fr_i64>(nb);
        fr_i64* slot_off = exact<fr_i64>(nb);
        fr_i64 at = 0, slots = 0;
        for (uint32_t s = 0; s < nb; s++) {
            len[s] = (int32_t)rd32(f, &ok);
            if (!ok || len[s] < 0 || len[s] > 65536) { ok = false; break; }
            off[s] = at; at += len[s];
            slot_off[s] = slots; slots += csv::fr_slot_size(len[s]);
        }
        if (!ok || at != (fr_i64)nbytes) { ok = false; break; }
        uint8_t* w = exact<uint8_t>(nbytes);
        if (nbytes && fread(w, 1, nbytes, f) != nbytes) { ok = false; break; }
        const csv::FrWin W{w, (fr_i64)nbytes, n_ref};
        const csv::FrOneLane L;
        fr_i64* g = exact<fr_i64>(nb);
        fr_i64* ex = exact<fr_i64>(nb);
        int32_t* cnt = exact<int32_t>(nb);
        int32_t* used = exact<int32_t>(nb);
        fr_i64* starts = exact<fr_i64>((size_t)slots);
        for (uint32_t s = 0; s < nb; s++) {                      // the guess pass: what one wavefront per block does
            const fr_i64 b = off[s], e = off[s] + len[s];
            g[s] = -1; ex[s] = -1; cnt[s] = 0;
            if (e <= (fr_i64)c) continue;                        // in front of the cursor
            g[s] = b <= (fr_i64)c ? (fr_i64)c : csv::fr_guess(L, W, b, e);
            if (g[s] >= 0) ex[s] = csv::fr_chase(W, g[s], e, starts + slot_off[s], csv::fr_slot_size(len[s]), &cnt[s]);
        }
        csv::FrStitch R;
        csv::fr_stitch(W, (int32_t)nb, off, len, slot_off, g, ex, cnt, starts, used, (fr_i64)c, &R);
        // the rows, in block order, against the naive walk
        std::vector<fr_i64> naive;
        fr_i64 o = c;
        while (o + 4 <= (fr_i64)nbytes) {
            int32_t bs;
            memcpy(&bs, w + o, 4);
            if (bs < 32 || o + 4 + (fr_i64)bs > (fr_i64)nbytes) break;
            naive.push_back(o);
            o += 4 + (fr_i64)bs;
        }
        uint64_t h = 1469598103934665603ull;
        size_t i = 0;
        bool same = R.tail == o && R.n_records == (fr_i64)naive.size();
        for (uint32_t s = 0; s < nb && same; s++)
            for (int32_t j = 0; j < used[s] && same; j++, i++) {
                const fr_i64 st = starts[slot_off[s] + j];
                if (i >= naive.size() || st != naive[i]) { same = false; break; }
                const csv::FrRow r = csv::fr_row(L, W, st);
                const uint8_t* p = (const uint8_t*)&r;
                for (size_t q = 0; q < sizeof r; q++) { h ^= p[q]; h *= 1099511628211ull; }
            }
        if (i != naive.size()) same = false;
        if (!same) { fprintf(stderr, "window %u: the core's record list is not the naive walk's (%lld records, tail %lld; naive %zu, %lld)\n", k, (long long)R.n_records, (long long)R.tail, naive.size(), (long long)o); bad++; }
        printf("%u %lld %lld %d %d %d %d %llu\n", k, (long long)R.n_records, (long long)R.tail, (int)R.tail_has_bs, R.tail_has_bs ? (int)R.tail_bs : 0, (int)R.right_blocks, (int)R.fallback_blocks,
               (unsigned long long)h);
        free(starts); free(used); free(cnt); free(ex); free(g); free(w); free(slot_off); free(off); free(len);
    }
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: truncated or malformed corpus\n", argv[1]); return 2; }
    return bad ? 1 : 0;
}
