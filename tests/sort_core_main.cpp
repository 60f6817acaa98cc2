// sort_core_main.cpp — cutesv_amd/csrc/sort_core.h on its own, for tests/test_bam_sort.py: built with -fsanitize=address,undefined
// and run as it is, nothing preloaded.
//   sort_core_main keys              one line per crafted record: refid pos flag n_ref refusal key
//   sort_core_main tiles             the tile rule on every tile size from 1 to 257 bytes over records of every length residue mod 16, in
//                                    three orders and with headers of several lengths: the reassembled stream must equal the concatenation
//   sort_core_main header IN OUT     the header rule: the BAM header in file IN, rewritten, into file OUT
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../cutesv_amd/csrc/sort_core.h"

using csv::so_i64;

static std::vector<uint8_t> record(int32_t refid, int32_t pos, uint16_t flag, so_i64 len, uint8_t fill)
{
    std::vector<uint8_t> r((size_t)len, fill);
    const int32_t bs = (int32_t)(len - 4);
    memcpy(r.data(), &bs, 4); memcpy(r.data() + 4, &refid, 4); memcpy(r.data() + 8, &pos, 4); memcpy(r.data() + 18, &flag, 2);
    return r;
}

static int run_keys()
{
    if (csv::sort_key_bits(2) != 0x7ffffffffull || csv::sort_key_bits(0) != 0x1ffffffffull || csv::sort_key_bits(300) != 0x3ffffffffffull) { fprintf(stderr, "bits\n"); return 1; }
    const int32_t n_ref = 300;
    const int32_t refids[] = {-2, -1, 0, 1, 255, 256, 299, 300, 2147483647, -2147483647 - 1};
    const int32_t poss[] = {-2147483647 - 1, -2, -1, 0, 1, (1 << 29) - 1, 1 << 29, 2147483646, 2147483647};
    const uint16_t flags[] = {0, 16, 4, 0xffef, 0xffff};
    for (int32_t refid : refids)
        for (int32_t pos : poss)
            for (uint16_t flag : flags) {
                const std::vector<uint8_t> r = record(refid, pos, flag, 36, 0xa5);
                const csv::SortFields f = csv::sort_fields(r.data());
                if (f.len != 36 || f.refid != refid || f.pos != pos || f.flag != flag) { fprintf(stderr, "fields\n"); return 1; }
                const int why = csv::sort_refuse(f, n_ref);
                const unsigned long long key = why ? 0ull : csv::sort_key(f, n_ref);
                if (!why && (key > csv::sort_key_bound(n_ref) || (key & ~csv::sort_key_bits(n_ref)))) { fprintf(stderr, "bound\n"); return 1; }
                printf("%d %d %u %d %d %llu\n", refid, pos, (unsigned)flag, n_ref, why, key);
            }
    return 0;
}

static int run_tiles()
{
    long long checked = 0;
    for (int hlen : {12, 16, 37, 300}) {
        std::vector<uint8_t> hdr((size_t)hlen);
        for (int i = 0; i < hlen; i++) hdr[(size_t)i] = (uint8_t)(200 + i);
        // records of every length residue mod 16 (36 .. 51 bytes), two longer than any tile, laid out in an arena behind a gap
        std::vector<uint8_t> arena(64, 0xee);
        std::vector<so_i64> starts;
        std::vector<so_i64> lens;
        for (int k = 0; k < 40; k++) {
            const so_i64 len = k == 7 ? 700 : k == 23 ? 1031 : 36 + (k % 16);
            const std::vector<uint8_t> r = record(k % 3, 1000 - k, (uint16_t)(k % 2 ? 16 : 0), len, (uint8_t)(k + 1));
            starts.push_back((so_i64)arena.size()); lens.push_back(len);
            arena.insert(arena.end(), r.begin(), r.end());
        }
        const so_i64 n = (so_i64)starts.size();
        for (int order = 0; order < 3; order++) {
            std::vector<int32_t> perm((size_t)n);
            for (so_i64 i = 0; i < n; i++) perm[(size_t)i] = (int32_t)(order == 1 ? n - 1 - i : (i * 7) % n);
            const int32_t* pp = order == 0 ? nullptr : perm.data();
            std::vector<so_i64> dst((size_t)n + 1, 0);
            std::vector<uint8_t> want(hdr);
            for (so_i64 r = 0; r < n; r++) {
                const so_i64 src = pp ? pp[r] : r;
                dst[(size_t)r + 1] = dst[(size_t)r] + lens[(size_t)src];
                want.insert(want.end(), arena.begin() + starts[(size_t)src], arena.begin() + starts[(size_t)src] + lens[(size_t)src]);
            }
            const so_i64 total = (so_i64)want.size();
            for (so_i64 r = 0; r < n; r++)                    // the search: every byte of every record names its record
                for (so_i64 x = dst[(size_t)r]; x < dst[(size_t)r + 1]; x += 5)
                    if (csv::sort_first_record(dst.data(), 0, n - 1, x) != r) { fprintf(stderr, "search %lld %lld\n", (long long)r, (long long)x); return 1; }
            for (so_i64 tile = 1; tile <= 257; tile++) {
                std::vector<uint8_t> got;
                for (so_i64 t0 = 0; t0 < total; t0 += tile) {
                    const so_i64 t1 = std::min(total, t0 + tile);
                    std::vector<uint8_t> piece((size_t)(t1 - t0));                 // (exactly the tile: the sanitizer sees a byte too many)
                    csv::sort_tile_fill(piece.data(), t0, t1, hdr.data(), hlen, arena.data(), starts.data(), pp, dst.data(), n);
                    got.insert(got.end(), piece.begin(), piece.end());
                    checked++;
                }
                if (got != want) { fprintf(stderr, "tile %lld header %d order %d\n", (long long)tile, hlen, order); return 1; }
            }
        }
        // no records at all: the stream is the header
        for (so_i64 tile = 1; tile <= 17; tile++) {
            std::vector<uint8_t> got((size_t)hlen);
            for (so_i64 t0 = 0; t0 < hlen; t0 += tile) csv::sort_tile_fill(got.data() + t0, t0, std::min<so_i64>(hlen, t0 + tile), hdr.data(), hlen, nullptr, nullptr, nullptr, nullptr, 0);
            if (got != hdr) { fprintf(stderr, "empty %lld\n", (long long)tile); return 1; }
        }
    }
    printf("tiles ok %lld\n", checked);
    return 0;
}

static int run_header(const char* in, const char* out)
{
    FILE* f = fopen(in, "rb");
    if (!f) return 2;
    std::vector<uint8_t> head;
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) head.insert(head.end(), buf, buf + k);
    fclose(f);
    std::vector<uint8_t> res;
    if (!csv::sort_header(head.data(), (so_i64)head.size(), &res)) { printf("refused\n"); return 0; }
    f = fopen(out, "wb");
    if (!f) return 2;
    fwrite(res.data(), 1, res.size(), f);
    fclose(f);
    printf("ok %zu\n", res.size());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !strcmp(argv[1], "keys")) return run_keys();
    if (argc == 2 && !strcmp(argv[1], "tiles")) return run_tiles();
    if (argc == 4 && !strcmp(argv[1], "header")) return run_header(argv[2], argv[3]);
    fprintf(stderr, "usage: sort_core_main keys | tiles | header IN OUT\n");
    return 2;
}
